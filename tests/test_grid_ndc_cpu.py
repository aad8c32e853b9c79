"""NDC cameras and the LLFF loader of the sparse voxel grid, the parts that need no GPU: the two grown structs and the new one
against the header, what the C entries refuse before they touch a device, the committed llff.json, the generated code of the
new kernel, and the numpy restatement of the warp against the reference's recorded bits."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_ndc_oracle as NO  # noqa: E402
from grid_testlib import assert_structs_match_c_header, compile_kernels_to_asm  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "grid_ndc.npz")
STRUCTS = {"nerf_grid_camera": "GridCamera", "nerf_grid_dataset_batch_args": "GridDatasetBatchArgs",
           "nerf_grid_rays_to_ndc_args": "GridRaysToNdcArgs"}


def test_grown_structs_match_a_c_compile_of_the_header(tmp_path):
    from nerf_projects_amd import _lib
    assert_structs_match_c_header(tmp_path, STRUCTS)
    # the sizes the header documents, and the new fields at the tail: a zeroed tail means no NDC
    assert C.sizeof(_lib.GridCamera) == 104 and _lib.GridCamera.ndc_coeffs.offset == 96
    assert _lib.GridCamera._fields_[-1][0] == "ndc_coeffs" and _lib.GridDatasetBatchArgs._fields_[-1][0] == "ndc_coeffs"
    assert _lib.GridDatasetBatchArgs.ndc_coeffs.offset == C.sizeof(_lib.GridDatasetBatchArgs) - 8
    assert list(_lib.GridCamera().ndc_coeffs) == [0.0, 0.0]


def _camera(_lib, ndc=(0.0, 0.0)):
    cam = _lib.GridCamera()
    cam.c2w[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    cam.fx = cam.fy = 10.0
    cam.cx, cam.cy, cam.width, cam.height = 4.0, 3.0, 8, 6
    cam.ndc_coeffs[:] = ndc
    return cam


BAD_COEFFS = ((float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 1.0), (1.0, float("inf")), (-float("inf"), 1.0),
              (1.0, 0.0), (1.0, -1.0), (-1.0, float("nan")))


def test_c_entries_refuse_bad_ndc_coeffs_before_any_device_call():
    """Every refusal here comes before a handle is dereferenced: the context and grid pointers are fakes."""
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "nerf_grid_rays_to_ndc") and "nerf_grid_rays_to_ndc" in _lib.EXPORTS
    fake = C.c_void_p(0x1000)
    err = lambda: lib.nerf_last_error().decode()      # noqa: E731
    ptr = C.c_void_p(8)
    for bad in BAD_COEFFS:
        cam = _camera(_lib, bad)
        assert lib.nerf_grid_gen_rays(fake, C.byref(cam), ptr, ptr, None) == -1 and "ndc_coeffs" in err(), bad
        opt, ra = _lib.GridRenderOptions(), _lib.GridRenderArgs()
        opt.step_size, ra.rgb = 0.5, 8
        assert lib.nerf_grid_render_image(fake, C.byref(cam), C.byref(opt), C.byref(ra)) == -1 and "ndc_coeffs" in err(), bad
        da = _lib.GridDepthArgs()
        assert lib.nerf_grid_depth_image(fake, C.byref(cam), C.byref(opt), C.byref(da)) == -1 and "ndc_coeffs" in err(), bad

        b = _lib.GridDatasetBatchArgs()
        b.n_images, b.height, b.width, b.channels, b.factor = 1, 4, 4, 3, 1
        b.fx = b.fy = 4.0
        b.n = 4
        b.images = b.c2w = b.origins = b.dirs = b.rgb = 8
        b.ndc_coeffs[:] = bad
        assert lib.nerf_grid_dataset_batch(fake, C.byref(b)) == -1 and "ndc_coeffs" in err(), bad

        a = _lib.GridRaysToNdcArgs()
        a.origins = a.dirs = a.origins_out = a.dirs_out = 8
        a.n = 4
        a.ndc_coeffs[:] = bad
        assert lib.nerf_grid_rays_to_ndc(fake, C.byref(a)) == -1 and "ndc_coeffs" in err(), bad
    # the kernel of its own has no "off": both coefficients must be positive
    a = _lib.GridRaysToNdcArgs()
    a.origins = a.dirs = a.origins_out = a.dirs_out = 8
    a.n = 4
    for off in ((0.0, 0.0), (-1.0, -1.0), (0.0, 2.0)):
        a.ndc_coeffs[:] = off
        assert lib.nerf_grid_rays_to_ndc(fake, C.byref(a)) == -1 and "must both be positive" in err(), off
    a.ndc_coeffs[:] = (1.0, 1.0)
    assert lib.nerf_grid_rays_to_ndc(None, C.byref(a)) == -1 and "NULL context" in err()
    assert lib.nerf_grid_rays_to_ndc(fake, None) == -1 and "NULL" in err()
    a.struct_size -= 8
    assert lib.nerf_grid_rays_to_ndc(fake, C.byref(a)) == -1 and "struct_size" in err()
    a = _lib.GridRaysToNdcArgs()
    a.ndc_coeffs[:] = (1.0, 1.0)
    a.origins = a.dirs = a.origins_out = a.dirs_out = 8
    for n in (-1, (1 << 26) + 1):
        a.n = n
        assert lib.nerf_grid_rays_to_ndc(fake, C.byref(a)) == -1 and "2^26" in err(), n
    a.n, a.dirs_out = 4, None
    assert lib.nerf_grid_rays_to_ndc(fake, C.byref(a)) == -1 and "dirs_out" in err()
    a.n = 0      # nothing to do: returns before the context is read
    assert lib.nerf_grid_rays_to_ndc(fake, C.byref(a)) == 0
    # a camera built against the header before ndc_coeffs (96 bytes) is refused by its size
    cam = _camera(_lib)
    cam.struct_size = 96
    assert lib.nerf_grid_gen_rays(fake, C.byref(cam), ptr, ptr, None) == -1 and "struct_size" in err()


def test_floater_and_background_entries_refuse_an_ndc_camera_before_any_device_call():
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x1000)
    err = lambda: lib.nerf_last_error().decode()      # noqa: E731
    cam = _camera(_lib, (1.5, 2.0))
    for fn, cls in ((lib.nerf_grid_floater_heatmap, _lib.GridFloaterHeatmapArgs), (lib.nerf_grid_component_view, _lib.GridComponentViewArgs)):
        a = cls()
        a.labels = a.table = 8
        a.radius[:] = [1.0, 1.0, 1.0]
        assert fn(fake, C.byref(cam), C.byref(a)) == -1 and "NDC camera" in err() and "pinhole" in err(), err()
    opt, b = _lib.GridRenderOptions(), _lib.GridBackgroundArgs()
    opt.step_size = 0.5
    b.rgb = b.log_transmit = 8
    assert lib.nerf_grid_background_image(fake, C.byref(cam), C.byref(opt), C.byref(b)) == -1 and "NDC camera" in err(), err()
    # ... and a camera with the tail zeroed, or svox2's (-1, -1), passes that check (it fails later, on its missing outputs)
    for off in ((0.0, 0.0), (-1.0, -1.0)):
        plain = _camera(_lib, off)
        a = _lib.GridComponentViewArgs()
        a.labels = a.table = 8
        a.radius[:] = [1.0, 1.0, 1.0]
        assert lib.nerf_grid_component_view(fake, C.byref(plain), C.byref(a)) == -1 and "keys and slots are required" in err()


def test_llff_json_parses_into_the_training_config():
    from nerf_projects_amd.grid_fit import GridTrainConfig
    cfg = GridTrainConfig.from_json(os.path.join(ROOT, "tests", "golden", "svox2_configs", "llff.json"))
    assert cfg.reso == [[256, 256, 128], [512, 512, 128], [1408, 1156, 128]]
    assert cfg.thresh_type == "sigma" and cfg.density_thresh == 5 and cfg.background_brightness == 0.5
    assert cfg.lambda_tv == 5e-4 and cfg.lambda_tv_sh == 5e-3 and cfg.lambda_sparsity == 1e-12 and cfg.tv_early_only == 0
    assert cfg.upsamp_every == 38400 and not cfg.last_sample_opaque


def test_python_side_refusals_need_no_device():
    import torch
    from nerf_projects_amd import Camera, NdcCamera
    c2w = torch.eye(4)[:3]
    for bad in ((-1.0, -1.0), (0.0, 1.0), (1.0, float("nan")), (float("inf"), 1.0), (1.0,), (1.0, 2.0, 3.0), "ab", None):
        with pytest.raises(ValueError, match="ndc_coeffs"):
            NdcCamera(c2w, 10.0, width=8, height=6, ndc_coeffs=bad)
    cam = NdcCamera(c2w, 10.0, 11.0, 4.0, 3.0, width=8, height=6, ndc_coeffs=[1.5, 2.0])
    assert isinstance(cam, Camera) and cam.using_ndc and cam.ndc_coeffs == (1.5, 2.0)
    c = cam._to_c()
    assert list(c.ndc_coeffs) == [1.5, 2.0] and (c.fx, c.fy, c.cx, c.cy, c.width, c.height) == (10.0, 11.0, 4.0, 3.0, 8, 6)
    assert list(Camera(c2w, 10.0, width=8, height=6)._to_c().ndc_coeffs) == [0.0, 0.0]
    with pytest.raises(NotImplementedError, match="NDC"):
        Camera(c2w, 10.0, width=8, height=6, ndc_coeffs=(1, 1))._to_c()


def test_ndc_kernel_uses_no_scratch_no_lds_and_no_inline_assembly(tmp_path):
    text, asm, build = compile_kernels_to_asm(tmp_path, "grid_ndc_kernels.hip")
    assert "grid_ndc_kernels.hip" in build.SOURCES
    assert not re.search(r"\basm\b|__asm", text)
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(kernels) == 1 and "grid_rays_to_ndc_kernel" in kernels[0], kernels
    assert [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)] == [0]
    assert [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)] == [0]
    body = asm[asm.index(kernels[0] + ":"):]
    assert "v_fma_f32" in body or "v_fmac_f32" in body      # the two fmas of the norm, and those of the divisions
    assert not re.search(r"\bv_rsq_f32|\bv_rcp_iflag", body)


def test_numpy_restatement_reproduces_the_reference_bits():
    """Pins the recipe on the CPU: the reference's NDC rays from its world rays, in every bit."""
    z = np.load(FIXTURE)
    assert os.path.getsize(FIXTURE) < 1 << 20
    coeffs = z["ndc_coeffs"]
    for f in (1, 2):
        o, d = NO.rays_to_ndc(z[f"world_origins_{f}"], z[f"world_dirs_{f}"], coeffs)
        assert np.array_equal(o, z[f"ndc_origins_{f}"]), f
        assert np.array_equal(d, z[f"ndc_dirs_{f}"]), f
    # (x x + y y) + z z, the other plausible norm, is not what the reference computes: the recipe is pinned, not incidental
    d32 = z["ndc_dirs_1"]
    o = z["world_origins_1"] + ((np.float32(1) - z["world_origins_1"][:, 2]) / z["world_dirs_1"][:, 2])[:, None] * z["world_dirs_1"]
    w = z["world_dirs_1"]
    raw = np.stack([np.float32(coeffs[0]) * (w[:, 0] / w[:, 2] - o[:, 0] / o[:, 2]),
                    np.float32(coeffs[1]) * (w[:, 1] / w[:, 2] - o[:, 1] / o[:, 2]), np.float32(2) / o[:, 2]], -1)
    plain = raw / np.sqrt((raw[:, 0] * raw[:, 0] + raw[:, 1] * raw[:, 1]) + raw[:, 2] * raw[:, 2])[:, None]
    assert plain.dtype == np.float32 and 0 < (plain != d32).any(-1).sum() < len(d32)
    # a ray parallel to the image plane comes back non-finite
    o, d = NO.rays_to_ndc(np.zeros((1, 3), np.float32), np.array([[1.0, 0.0, 0.0]], np.float32), coeffs)
    assert not np.isfinite(o).all() and not np.isfinite(d).all()


def test_fixture_is_what_the_issue_asks_for():
    z = np.load(FIXTURE)
    assert z["c2w"].shape == (4, 4, 4) and tuple(z["hw_full"]) == (8, 12) and tuple(z["hw_2"]) == (4, 6)
    assert z["ndc_origins_1"].shape == (384, 3) and z["ndc_origins_2"].shape == (96, 3)
    assert z["test_c2w_hold8"].shape[0] == 1 and z["test_c2w_hold2"].shape[0] == 3 and z["train_c2w_hold2"].shape[0] == 2
    assert z["render_c2w_hold8"].shape == (120, 4, 4)
    assert tuple(z["cam4_size"]) == (13, 9) and z["cam4_intrinsics"][0] != z["cam4_intrinsics"][1]
    assert tuple(z["grid_reso"]) == (12, 10, 6)
    for tag in ("train", "cam4"):
        assert (z[f"render_{tag}_opacity64"] > 0.1).mean() >= 0.5
    assert np.allclose(np.linalg.norm(z["ndc_dirs_1"], axis=-1), 1.0, atol=1e-6)
