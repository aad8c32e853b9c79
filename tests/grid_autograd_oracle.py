"""numpy fp32 restatement of the sparse voxel grid's gradients for autograd (include/nerf_mi355x.h, "Sparse voxel grid:
gradients for autograd"): the taped render, the render backward with a cotangent supplied from outside, and the transpose of
the sampler - every operation a separate fp32 rounding in the order the header states, `remaining` in fp64. It builds on
grid_oracle.march_colour and grid_train_oracle.march_colour_bwd (same grid dict) and, like them, is a test oracle: slow and simple. Sums into a gradient row are
taken in sample order (the kernels' atomics take them in any order), so gradients agree with the kernels to rounding of those
sums.
"""
import functools

import numpy as np

import grid_oracle as GO
import grid_train_oracle as GT

F = GO.F


def render_taped(grid, origins, dirs, step_size=0.5, sigma_thresh=1e-10, stop_thresh=1e-7, background_brightness=1.0,
                 near_clip=0.0, skip=None):
    """rgb [N, 3] fp32 (the render's), log_transmit [N], tape [N, 3] fp64"""
    rgb, log_t, (_, _, _, tape), _ = GO.march_colour(grid, origins, dirs, step_size, sigma_thresh, stop_thresh, near_clip, skip)
    bg = np.exp(log_t).astype(F)
    rgb = (rgb + (bg * F(background_brightness))[:, None]).astype(F)
    tape = tape + (bg.astype(np.float64) * np.float64(F(background_brightness)))[:, None]
    return rgb, log_t, tape


def render_backward(grid, origins, dirs, grad_rgb, tape, step_size=0.5, sigma_thresh=1e-10, stop_thresh=1e-7,
                    near_clip=0.0, skip=None, grad_density=None, grad_sh=None, mask=None):
    """grad_density [C, 1], grad_sh [C, 3 B], mask [C] uint8 of ``sum(grad_rgb * rgb)``; added to when passed in"""
    gd, gs, mk = GT.grad_tables(grid, grad_density, grad_sh, mask)
    gc = np.asarray(grad_rgb, F)
    if gc.shape[0] == 0:
        return gd, gs, mk
    Y, delta_scale = GO.view_bases(grid, origins, dirs, near_clip)
    # (remaining: a copy of the tape, reduced sample by sample)
    shade = functools.partial(GT.march_colour_bwd, gc=gc, remaining=np.array(tape, dtype=np.float64), Y=Y,
                              step_ds=(F(step_size) * delta_scale).astype(F), grad_density=gd, grad_sh=gs, mask=mk)
    with np.errstate(over="ignore", invalid="ignore"):
        GO.march_colour(grid, origins, dirs, step_size, sigma_thresh, stop_thresh, near_clip, skip, shade=shade)
    return gd, gs, mk


def render_vjp(grid, origins, dirs, grad_rgb, background_brightness=1.0, **kw):
    """taped render, then the backward with ``grad_rgb(rgb)`` (a callable) or ``grad_rgb`` (an array): rgb, gd, gs, mask"""
    fwd = {k: v for k, v in kw.items() if k in ("step_size", "sigma_thresh", "stop_thresh", "near_clip", "skip")}
    rgb, _, tape = render_taped(grid, origins, dirs, background_brightness=background_brightness, **fwd)
    g = grad_rgb(rgb) if callable(grad_rgb) else grad_rgb
    return (rgb,) + render_backward(grid, origins, dirs, g, tape, **kw)


def sample_backward(grid, points, grad_out_density, grad_out_sh=None, grid_coords=False, want_colors=True,
                    grad_density=None, grad_sh=None):
    """The transpose of grid_oracle.sample: every kept corner's row receives ((w_x * go) * w_y) * w_z."""
    links = grid["links"]
    cap, cols = grid["density_data"].shape[0], grid["sh_data"].shape[1]
    gd = np.zeros((cap, 1), dtype=F) if grad_density is None else grad_density
    gs = np.zeros((cap, cols), dtype=F) if grad_sh is None else grad_sh
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    if not grid_coords:
        offset, scaling, _ = GO.world2grid_consts(grid)
        p = (offset + p * scaling).astype(F)
    l, wb = GO._cell(p, links.shape)
    wa = (F(1.0) - wb).astype(F)
    lk = GO._corner_links(links, l)
    go_d = np.asarray(grad_out_density, F).reshape(-1, 1)
    go_s = np.asarray(grad_out_sh, F).reshape(-1, cols) if want_colors else None
    for c in range(8):
        wx = (wb if c & 4 else wa)[:, 0:1]
        wy = (wb if c & 2 else wa)[:, 1:2]
        wz = (wb if c & 1 else wa)[:, 2:3]
        kept = (lk[c] >= 0) & (lk[c] < cap)
        rows = lk[c][kept]
        np.add.at(gd, rows, (((wx * go_d).astype(F) * wy).astype(F) * wz).astype(F)[kept])
        if want_colors:
            np.add.at(gs, rows, (((wx * go_s).astype(F) * wy).astype(F) * wz).astype(F)[kept])
    return gd, gs
