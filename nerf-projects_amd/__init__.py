"""MI355X-native NeRF ray-chunk renderer.

Drop-in for the render path of isaacchunn/nerf-projects ``nerf/`` (``render_rays`` /
``raw2outputs`` / ``run_network`` / ``render`` ...): see DESIGN.md and INTEGRATION.md.
Importing the package never touches the GPU; the first call that needs it loads
``libnerf_mi355x.so`` and raises if the library or a gfx950 device is missing.
"""
from . import synthetic  # noqa: F401
from .host import (Adam, NeRF, NetworkQuery, train_on_batch, batchify, batchify_rays, calculate_lpips, calculate_metrics,  # noqa: F401
                   calculate_ssim, create_nerf, generate_rays, get_context, get_embedder, get_rays, get_rays_np,
                   img2mse, load_checkpoint, make_network_query_fn, mse2psnr, ndc_rays, pack_rays, raw2outputs,
                   render, render_path, render_rays, render_shard, run_network, sample_pdf, save_checkpoint, to8b, write_png)
from . import datasets  # noqa: F401
from .datasets import load_blender_data, load_llff_data, read_png  # noqa: F401
from .sharded import ensure_ipc_env, gather_frame, render_sharded, shard_bounds  # noqa: F401
from .batching import RayBatcher  # noqa: F401
from .mesh import density_grid, marching_cubes, marching_cubes_volume, save_obj  # noqa: F401
from .occupancy import OccupancyGrid  # noqa: F401
from . import grid  # noqa: F401
from .grid import Camera, NdcCamera, Rays, RenderOptions, SparseGrid, rays_to_ndc  # noqa: F401
from . import grid_half  # noqa: F401
from .grid_half import HalfGrid  # noqa: F401
from . import grid_palette  # noqa: F401
from .grid_palette import PaletteGrid, quantize_median_cut  # noqa: F401
from . import grid_background  # noqa: F401
from .grid_background import BackgroundGrid, load_grid  # noqa: F401
from . import grid_train  # noqa: F401
from .grid_train import GridTrainer  # noqa: F401
from . import grid_background_train  # noqa: F401
from .grid_background_train import BackgroundTrainer  # noqa: F401
from . import grid_autograd  # noqa: F401
from .grid_autograd import GridModule  # noqa: F401
from . import grid_resample  # noqa: F401
from .grid_resample import dilate_mask, resample_grid, weight_render  # noqa: F401
from . import grid_components  # noqa: F401
from .grid_components import (compute_all_advanced_metrics, compute_FDR, compute_MCQ, label_components,  # noqa: F401
                              remove_floaters)
from . import grid_floater_views  # noqa: F401
from .grid_floater_views import (component_view, floater_overlay_on_render, main_object_overlay, multi_object_overlay,  # noqa: F401
                                 project_floaters_to_view)
from . import grid_dataset  # noqa: F401
from .grid_dataset import GridDataset  # noqa: F401
from . import grid_mesh  # noqa: F401
from .grid_mesh import GridMesh, extract_mesh, mesh_attributes  # noqa: F401
from . import grid_fit  # noqa: F401
from .grid_fit import GridTrainConfig, expon_lr, train_grid  # noqa: F401
from . import octree  # noqa: F401
from .octree import N3Tree  # noqa: F401
from . import octree_optimize  # noqa: F401

__version__ = "0.1.0"
