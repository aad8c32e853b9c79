#!/usr/bin/env python3
"""Benchmark of the palette-quantised sparse voxel grid (PaletteGrid) against the fp32 grid it was made from and its HalfGrid,
on one MI355X.

    python bench_grid_palette.py [--steps 20] [--warmup 3] [--reso 128 256] [--hw 800] [--out profiles/grid_palette.md]

The scene of bench_grid.py: the network of bench.py (synthetic_pair(0), 8 x 256, view directions) baked with
SparseGrid.from_nerf(fine, -1.5, 1.5, R), basis_dim 9, and the 800 x 800 lego camera. Legs, all after accelerate(), alternated
step by step in one process and timed with HIP events on the current stream after warm-up:
  float          SparseGrid.volume_render_image(camera)                  108 B of colour per node
  half           HalfGrid().volume_render_image(camera)                  64 B
  p16r0, p16r1   PaletteGrid(bits=16, retain=0 / 1)                      18 B / 22 B, palettes of 65 536 entries
  p12r0, p12r1   PaletteGrid(bits=12, retain=0 / 1)                      the same indices, palettes of 4 096 entries
Per R and leg: the resident bytes, the compression time (from_grid, one run, host clock around a synchronise), the median frame
time, its ratio to the half leg's per step (median and spread: in one process, on the same steps), the PSNR of the frame against
the fp32 grid's frame, and the check that the palette frame IS the fp32 frame of the dequantised table, bit for bit. Prints
one JSON line and writes the table to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PALETTES = (("p16r0", 16, 0), ("p16r1", 16, 1), ("p12r0", 12, 0), ("p12r1", 12, 1))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reso", type=int, nargs="+", default=[128, 256])
    p.add_argument("--n-dirs", type=int, default=64)
    p.add_argument("--box", type=float, default=1.5)
    p.add_argument("--hw", type=int, default=800)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_palette.md"))
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0:
        p.error("--steps >= 1 and --warmup >= 0 are required")
    torch.cuda.set_device(0)
    import nerf_projects_amd as N
    from nerf_projects_amd import _lib, synthetic
    arch = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    _, sd_f = synthetic.synthetic_pair(0)
    net_f = N.NeRF(**arch).load_state_dict(sd_f)
    H = W = a.hw
    K, c2w, _, _ = synthetic.lego_camera(H, W)
    cam = N.Camera.from_nerf_pose(c2w, H, W, float(K[0][0]))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    def psnr(img, ref):
        mse = float(((img.double() - ref.double()) ** 2).mean())
        return float("inf") if mse == 0.0 else float(-10.0 * np.log10(mse))

    legs = ("float", "half") + tuple(name for name, _, _ in PALETTES)
    out = {"metric": "grid_palette_frame", "frame": f"lego {H}x{W}, synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], "
           f"basis_dim 9, n_dirs {a.n_dirs}, step_size 0.5, after accelerate()", "steps": a.steps, "warmup": a.warmup,
           "library": os.path.basename(_lib.library_path()), "grids": {}}
    for R in a.reso:
        src = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
        grids, res = {"float": src, "half": src.to_half()}, {"kept_nodes": src.capacity, "kept_fraction": src.capacity / src.links.numel()}
        shared = src.links.numel() * 4 + src.density_data.numel() * 4
        res["float_bytes_resident"] = shared + src.sh_data.numel() * 4
        res["half_bytes_resident"] = shared + grids["half"].sh_bytes
        for name, bits, retain in PALETTES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grids[name] = src.to_palette(bits=bits, retain=retain)
            torch.cuda.synchronize()
            res[f"{name}_compress_s"] = time.perf_counter() - t0
            res[f"{name}_bytes_resident"] = grids[name].bytes_resident
            res[f"{name}_sh_bytes"] = grids[name].sh_bytes
        for g in grids.values():
            g.accelerate()
        times = {leg: [] for leg in legs}
        for step in range(a.warmup + a.steps):
            for leg in legs:
                ms, _ = timed(lambda: grids[leg].volume_render_image(cam))
                if step >= a.warmup:
                    times[leg].append(ms)
        for leg in legs:
            res[f"{leg}_ms"] = float(np.median(times[leg]))
            res[f"{leg}_ms_min"] = float(np.min(times[leg]))
            ratio = np.array(times[leg]) / np.array(times["half"])      # per step: the two frames ran back to back
            res[f"{leg}_over_half"] = float(np.median(ratio))
            res[f"{leg}_over_half_min"], res[f"{leg}_over_half_max"] = float(ratio.min()), float(ratio.max())
        ref = src.volume_render_image(cam)
        res["half_psnr_db"] = psnr(grids["half"].volume_render_image(cam), ref)
        for name, _, _ in PALETTES:
            img = grids[name].volume_render_image(cam)
            deq = grids[name].to_float()
            deq.accelerate()
            assert torch.equal(img, deq.volume_render_image(cam)), name      # lossless on the tables it holds
            res[f"{name}_psnr_db"] = psnr(img, ref)
            del deq
        res["pixels"] = H * W
        out["grids"][str(R)] = res
        del grids, src
        torch.cuda.empty_cache()
    print(json.dumps(out))
    lines = ["# PaletteGrid: frame time, bytes and quality against the fp32 grid and HalfGrid", "",
             f"`python bench_grid_palette.py --steps {a.steps} --warmup {a.warmup} --reso {' '.join(map(str, a.reso))} --hw {a.hw}` "
             f"on one MI355X: {out['frame']}. One process, the legs alternated step by step; `x half` is the per-step ratio to the "
             "HalfGrid frame of the same step (median, and its least and greatest value over the steps).", ""]
    for R, res in out["grids"].items():
        lines += [f"## R = {R}: {res['kept_nodes']} kept nodes ({100 * res['kept_fraction']:.1f} %)", "",
                  "| leg | resident MB | frame ms (median) | x half (median, min - max) | PSNR vs fp32 frame, dB | compress s |",
                  "|---|---|---|---|---|---|"]
        for leg in legs:
            quality = "-" if leg == "float" else f"{res[f'{leg}_psnr_db']:.2f}"
            compress = f"{res[f'{leg}_compress_s']:.2f}" if f"{leg}_compress_s" in res else "-"
            lines.append(f"| {leg} | {res[f'{leg}_bytes_resident'] / 1e6:.1f} | {res[f'{leg}_ms']:.3f} | {res[f'{leg}_over_half']:.3f} "
                         f"({res[f'{leg}_over_half_min']:.3f} - {res[f'{leg}_over_half_max']:.3f}) | {quality} | {compress} |")
        lines.append("")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
