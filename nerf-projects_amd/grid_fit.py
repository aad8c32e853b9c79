"""Training a sparse voxel grid from a dataset: the loop of svox2's ``opt/opt.py`` around the HIP kernels of
:class:`~nerf_projects_amd.grid_train.GridTrainer`, with ``opt.py``'s option names and defaults.

    dset = GridDataset.from_blender(scene_dir, "train", epoch_size=12800 * 5000, permutation=False)
    test = GridDataset.from_blender(scene_dir, "test")
    grid, history = train_grid(dset, GridTrainConfig.from_json("configs/syn.json"), test=test)

What ``opt.py`` does per step and per epoch is kept: the two exponential learning-rate schedules (:func:`expon_lr`), the
fused render + backward, the TV gradients while their weights are not 0, the masked RMSProp step once
``lr_fg_begin_step`` is reached, and after an epoch that crosses ``upsamp_every`` the TV rule (``tv_early_only`` /
``tv_decay``), ``resample`` to the next resolution and ``upsample_density_add``. Three things differ. The data side is
:class:`~nerf_projects_amd.grid_dataset.GridDataset`: a batch is one launch, nothing is shuffled on the host. The step waits
for nothing: ``opt.py`` reads the batch MSE every step (``.item()``); here it is added into a device scalar that is read every
``print_every`` steps and at an epoch's end. And training stops AT ``n_iters``: ``opt.py`` only looks at the end of an epoch
and may overshoot by most of one. TensorBoard, checkpoints, SSIM / LPIPS and the background model are not part of the driver.
"""
import json
import math
from dataclasses import dataclass, field, fields
from typing import Any, List

import torch

from .grid import SparseGrid
from .grid_train import GridTrainer

__all__ = ["GridTrainConfig", "expon_lr", "train_grid", "evaluate"]

# opt.py / config_util options that have no effect on this driver: logging and checkpoint cadence, the parameters of models
# that are refused before they could be read (background layers, learned bases), and the data options, which belong to the
# GridDataset. They are accepted in a configuration file and dropped.
_IGNORED = frozenset("""
    train_dir config data_dir save_every log_mse_image log_depth_map log_depth_map_use_thresh log_advanced_metrics
    advanced_metrics_every log_fdr fdr_every log_floater_viz floater_viz_slices fdr_density_threshold
    fdr_main_object_threshold log_density_render tune_mode tune_nosave n_train tv_contiguous weight_decay_sigma
    weight_decay_sh background_reso background_density_thresh init_sigma_bg bg_optim lr_sigma_bg lr_sigma_bg_final
    lr_sigma_bg_decay_steps lr_sigma_bg_delay_steps lr_sigma_bg_delay_mult lr_color_bg lr_color_bg_final
    lr_color_bg_decay_steps lr_color_bg_delay_steps lr_color_bg_delay_mult lambda_tv_background_sigma
    lambda_tv_background_color tv_background_sparsity basis_reso mlp_posenc_size mlp_width basis_optim lr_basis
    lr_basis_final lr_basis_decay_steps lr_basis_delay_steps lr_basis_begin_step lr_basis_delay_mult
    tv_lumisphere_sparsity tv_lumisphere_dir_factor random_sigma_std random_sigma_std_background
    dataset_type scene_scale scale seq_id epoch_size white_bkgd llffhold normalize_by_bbox data_bbox_scale
    cam_scale_factor normalize_by_camera perm
""".split())


def _default_reso():
    return [[256, 256, 256], [512, 512, 512]]


@dataclass
class GridTrainConfig:
    """``opt.py``'s options (and ``config_util``'s render options) under their names, with their defaults."""
    reso: List[Any] = field(default_factory=_default_reso)
    upsamp_every: int = 3 * 12800
    init_iters: int = 0
    upsample_density_add: float = 0.0
    basis_type: str = "sh"
    sh_dim: int = 9
    background_nlayers: int = 0
    n_iters: int = 10 * 12800
    batch_size: int = 5000
    sigma_optim: str = "rmsprop"
    lr_sigma: float = 3e1
    lr_sigma_final: float = 5e-2
    lr_sigma_decay_steps: int = 250000
    lr_sigma_delay_steps: int = 15000
    lr_sigma_delay_mult: float = 1e-2
    sh_optim: str = "rmsprop"
    lr_sh: float = 1e-2
    lr_sh_final: float = 5e-6
    lr_sh_decay_steps: int = 250000
    lr_sh_delay_steps: int = 0
    lr_sh_delay_mult: float = 1e-2
    lr_fg_begin_step: int = 0
    lr_decay: bool = True
    rms_beta: float = 0.95
    print_every: int = 20
    eval_every: int = 1
    init_sigma: float = 0.1
    thresh_type: str = "weight"
    weight_thresh: float = 0.0005 * 512
    density_thresh: float = 5.0
    max_grid_elements: int = 44_000_000
    lambda_tv: float = 1e-5
    tv_sparsity: float = 0.01
    tv_logalpha: bool = False
    lambda_tv_sh: float = 1e-3
    tv_sh_sparsity: float = 0.01
    lambda_tv_lumisphere: float = 0.0
    lambda_l2_sh: float = 0.0
    lambda_tv_basis: float = 0.0
    tv_decay: float = 1.0
    tv_early_only: int = 1
    lambda_sparsity: float = 0.0
    lambda_beta: float = 0.0
    nosphereinit: bool = False
    # config_util.define_common_args, "Render options"
    step_size: float = 0.5
    sigma_thresh: float = 1e-8
    stop_thresh: float = 1e-7
    background_brightness: float = 1.0
    near_clip: float = 0.0
    renderer_backend: str = "cuvol"
    use_spheric_clip: bool = False
    enable_random: bool = False
    last_sample_opaque: bool = False

    def __post_init__(self):
        if isinstance(self.reso, str):      # opt.py takes the list as a JSON string
            self.reso = json.loads(self.reso)
        if isinstance(self.reso, int):
            self.reso = [self.reso]
        self.validate()

    def validate(self):
        """``NotImplementedError`` naming an option this package does not build; ``ValueError`` for a value out of range."""
        refused = (("background_nlayers", self.background_nlayers > 0, "background layers are trained by BackgroundTrainer, not by this driver"),
                   ("renderer_backend", self.renderer_backend != "cuvol", "only the cuvol renderer is built"),
                   ("last_sample_opaque", bool(self.last_sample_opaque), "not built"),
                   ("enable_random", bool(self.enable_random), "sigma noise is not built"),
                   ("use_spheric_clip", bool(self.use_spheric_clip), "not built"),
                   ("tv_logalpha", bool(self.tv_logalpha), "not built"),
                   ("basis_type", self.basis_type != "sh", "only spherical harmonics are built"),
                   ("lambda_tv_lumisphere", self.lambda_tv_lumisphere > 0, "not built"),
                   ("lambda_l2_sh", self.lambda_l2_sh > 0, "not built"),
                   ("lambda_tv_basis", self.lambda_tv_basis > 0, "learned bases are not built"))
        for name, bad, why in refused:
            if bad:
                raise NotImplementedError(f"{name} = {getattr(self, name)!r}: {why}")
        if self.sigma_optim != self.sh_optim:
            raise NotImplementedError(f"sigma_optim = {self.sigma_optim!r} with sh_optim = {self.sh_optim!r}: GridTrainer.step "
                                      "takes one optimiser for both tables")
        if self.sigma_optim not in ("rmsprop", "sgd"):
            raise ValueError(f"sigma_optim = {self.sigma_optim!r}: 'rmsprop' or 'sgd'")
        if self.thresh_type not in ("weight", "sigma"):
            raise ValueError(f"thresh_type = {self.thresh_type!r}: 'weight' or 'sigma'")
        if not isinstance(self.reso, (list, tuple)) or not self.reso:
            raise ValueError(f"reso = {self.reso!r} must be a non-empty list of resolutions")
        for name in ("upsamp_every", "n_iters", "batch_size", "print_every"):
            if int(getattr(self, name)) < 1:
                raise ValueError(f"{name} = {getattr(self, name)!r} must be at least 1")
        if self.lr_sigma_final > self.lr_sigma or self.lr_sh_final > self.lr_sh:
            raise ValueError("lr_sigma must be >= lr_sigma_final and lr_sh >= lr_sh_final")

    @classmethod
    def from_dict(cls, options):
        known = {f.name for f in fields(cls)}
        unknown = sorted(set(options) - known - _IGNORED)
        if unknown:
            raise ValueError(f"unknown option{'s' if len(unknown) > 1 else ''} {unknown}")
        return cls(**{k: v for k, v in options.items() if k in known})

    @classmethod
    def from_json(cls, path):
        """A svox2 configuration file (``opt/configs/*.json``): its keys override the defaults. An unknown key is an error."""
        with open(path) as f:
            return cls.from_dict(json.load(f))


def expon_lr(step, lr_init, lr_final, delay_steps=0, delay_mult=1.0, max_steps=1000000):
    """The value of svox2's ``get_expon_lr_func(lr_init, lr_final, delay_steps, delay_mult, max_steps)(step)``: log-linear
    from ``lr_init`` at step 0 to ``lr_final`` at ``max_steps`` (constant after), times, with ``delay_steps > 0``, the ramp
    ``delay_mult + (1 - delay_mult) sin(pi / 2 * clip(step / delay_steps, 0, 1))``. 0 for a negative step or two zero rates."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    ramp = 1.0
    if delay_steps > 0:
        ramp = delay_mult + (1.0 - delay_mult) * math.sin(0.5 * math.pi * min(max(step / delay_steps, 0.0), 1.0))
    t = min(max(step / max_steps, 0.0), 1.0)
    return ramp * math.exp(math.log(lr_init) * (1.0 - t) + math.log(lr_final) * t)


def evaluate(grid, dataset, n_images=None):
    """``{"mse", "psnr", "n_images"}``: ``opt.py``'s evaluation pass without its image logging. ``n_images`` evenly spaced
    views of ``dataset`` (``range(0, n, n // n_images)``, all by default) are rendered with ``volume_render_image`` and
    compared with ``dataset.image(i)``; the per-image MSE and PSNR are averaged. Waits for the device once per image."""
    n = dataset.n_images
    k = n if n_images is None else max(1, min(int(n_images), n))
    ids = range(0, n, n // k)
    mse_sum = psnr_sum = 0.0
    with torch.no_grad():
        for i in ids:
            pred = grid.volume_render_image(dataset.camera(i))
            mse = float(((dataset.image(i) - pred) ** 2).mean())
            mse_sum += mse
            psnr_sum += -10.0 * math.log10(mse) if mse > 0 else float("inf")
    return {"mse": mse_sum / len(ids), "psnr": psnr_sum / len(ids), "n_images": len(ids)}


def _z_reso(reso):
    return reso if isinstance(reso, int) else reso[2]


def train_grid(dataset, config, test=None, generator=None, on_eval=None, trainer_factory=GridTrainer, grid_factory=SparseGrid):
    """Runs ``opt.py``'s schedule and returns ``(grid, history)``.

    ``dataset``: a :class:`~nerf_projects_amd.grid_dataset.GridDataset` (anything with ``shuffle_rays``, ``n_rays``,
    ``batch``, ``camera``, ``n_images``, ``scene_center``, ``scene_radius``, ``use_sphere_bound``). ``config``: a
    :class:`GridTrainConfig`; it is not modified (the TV weights that ``opt.py`` changes in its ``args`` are locals here).
    ``test``: a dataset evaluated at the start of every ``eval_every``-th epoch (5 views in the first epoch, 20 later, as
    ``opt.py``) and after the last step; ``on_eval(entry)`` is called with every such history entry. ``generator``: the CPU
    ``torch.Generator`` of the trainer's TV cell ranges. ``trainer_factory(grid, generator=...)`` makes the trainer and
    ``grid_factory(**svox2's SparseGrid arguments)`` the initial grid (the tests record the schedule through them).

    ``history`` holds, in order, ``{"kind": "train", "step", "mse", "psnr"}`` - the mean batch MSE since the last entry, read
    from the device every ``print_every`` steps and at an epoch's end, which are the only waits of the loop besides
    ``resample`` - and ``{"kind": "eval", "step", "epoch", "mse", "psnr", "n_images"}``."""
    cfg = config
    cfg.validate()
    reso_list = list(cfg.reso)
    grid = grid_factory(reso=reso_list[0], center=dataset.scene_center, radius=dataset.scene_radius,
                        use_sphere_bound=bool(dataset.use_sphere_bound and not cfg.nosphereinit), basis_dim=cfg.sh_dim,
                        use_z_order=True, device=getattr(dataset, "device", "cuda"))
    grid.sh_data.zero_()      # DC -> gray
    grid.density_data.fill_(0.0 if cfg.lr_fg_begin_step > 0 else cfg.init_sigma)
    opt = grid.opt
    opt.step_size, opt.sigma_thresh, opt.stop_thresh = cfg.step_size, cfg.sigma_thresh, cfg.stop_thresh
    opt.background_brightness, opt.near_clip = cfg.background_brightness, cfg.near_clip
    trainer = trainer_factory(grid, generator=generator)
    cameras = [dataset.camera(i) for i in range(dataset.n_images)] if cfg.thresh_type == "weight" else None
    lambda_tv, lambda_tv_sh = cfg.lambda_tv, cfg.lambda_tv_sh
    use_losses = bool(cfg.lambda_beta or cfg.lambda_sparsity)
    history = []

    def eval_entry(step, epoch):
        if test is None:
            return
        entry = {"kind": "eval", "step": step, "epoch": epoch, **evaluate(grid, test, 20 if epoch > 0 else 5)}
        history.append(entry)
        if on_eval is not None:
            on_eval(entry)

    loss = {"sum": None, "steps": 0}

    def read_loss(step):
        if not loss["steps"]:
            return
        mse = float(loss["sum"]) / loss["steps"]      # the wait
        history.append({"kind": "train", "step": step, "mse": mse, "psnr": -10.0 * math.log10(mse) if mse > 0 else float("inf")})
        loss["sum"].zero_()
        loss["steps"] = 0

    step_base, last_upsamp, reso_id, epoch = 0, cfg.init_iters, 0, -1
    while True:
        dataset.shuffle_rays()
        epoch += 1
        epoch_size = dataset.n_rays
        if epoch % max(1, cfg.eval_every) == 0:
            eval_entry(step_base, epoch)
        done = 0
        for iter_id, begin in enumerate(range(0, epoch_size, cfg.batch_size)):
            step = step_base + iter_id
            if step >= cfg.n_iters:
                break
            if cfg.lr_fg_begin_step > 0 and step == cfg.lr_fg_begin_step:
                grid.density_data.fill_(cfg.init_sigma)
            if cfg.lr_decay:
                lr_sigma = expon_lr(step, cfg.lr_sigma, cfg.lr_sigma_final, cfg.lr_sigma_delay_steps, cfg.lr_sigma_delay_mult,
                                    cfg.lr_sigma_decay_steps)
                lr_sh = expon_lr(step, cfg.lr_sh, cfg.lr_sh_final, cfg.lr_sh_delay_steps, cfg.lr_sh_delay_mult, cfg.lr_sh_decay_steps)
            else:
                lr_sigma, lr_sh = cfg.lr_sigma, cfg.lr_sh
            rays, rgb_gt = dataset.batch(begin, min(begin + cfg.batch_size, epoch_size))
            trainer.zero_grad()
            if use_losses:
                rgb = trainer.volume_render_fused(rays, rgb_gt, beta_loss=cfg.lambda_beta, sparsity_loss=cfg.lambda_sparsity)
            else:
                rgb = trainer.forward_backward(rays, rgb_gt)
            mse = ((rgb - rgb_gt) ** 2).mean()      # stays on the device
            loss["sum"] = mse if loss["sum"] is None else loss["sum"].add_(mse)
            loss["steps"] += 1
            if (iter_id + 1) % cfg.print_every == 0:
                read_loss(step)
            if lambda_tv > 0.0:
                trainer.add_tv_grad("density", lambda_tv, cfg.tv_sparsity)
            if lambda_tv_sh > 0.0:
                trainer.add_tv_grad("sh", lambda_tv_sh, cfg.tv_sh_sparsity, ignore_edge=True)
            if step >= cfg.lr_fg_begin_step:
                trainer.step(lr_sigma, lr_sh, beta=cfg.rms_beta, optim=cfg.sigma_optim)
            done = iter_id + 1
        step_base += done
        read_loss(step_base - 1)
        if step_base - last_upsamp >= cfg.upsamp_every:
            last_upsamp = step_base
            if reso_id < len(reso_list) - 1:
                if cfg.tv_early_only > 0:
                    lambda_tv = lambda_tv_sh = 0.0
                elif cfg.tv_decay != 1.0:
                    lambda_tv *= cfg.tv_decay
                    lambda_tv_sh *= cfg.tv_decay
                reso_id += 1
                trainer.resample(reso_list[reso_id], sigma_thresh=cfg.density_thresh,
                                 weight_thresh=cfg.weight_thresh / _z_reso(reso_list[reso_id]), dilate=2, cameras=cameras,
                                 max_elements=cfg.max_grid_elements)
                if cfg.upsample_density_add:
                    grid.density_data.add_(cfg.upsample_density_add)
        if step_base >= cfg.n_iters:
            eval_entry(step_base, epoch)
            return grid, history
