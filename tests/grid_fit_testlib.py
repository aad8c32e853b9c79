"""What the CPU and the GPU test of ``train_grid`` share: recorders for the trainer and the dataset, and the schedule that
``opt.py``'s rules give for a configuration, written out step by step. A plain module (no fixtures, no pytest settings)."""
from nerf_projects_amd.grid_fit import expon_lr

RESO = [[8, 8, 8], [16, 16, 16]]


def recording_trainer(base, events):
    """A subclass of ``base`` (``GridTrainer`` or a stand-in) whose training calls are appended to ``events`` before they run."""

    class Recording(base):
        def zero_grad(self):
            events.append(("zero_grad",))
            return super().zero_grad()

        def forward_backward(self, rays, rgb_gt, **kw):
            events.append(("forward_backward", int(rays.origins.shape[0]), kw))
            return super().forward_backward(rays, rgb_gt, **kw)

        def volume_render_fused(self, rays, rgb_gt, **kw):
            events.append(("volume_render_fused", int(rays.origins.shape[0]), kw))
            return super().volume_render_fused(rays, rgb_gt, **kw)

        def add_tv_grad(self, target, scaling, sparse_frac, ignore_edge=False):
            events.append(("add_tv_grad", target, scaling, sparse_frac, ignore_edge))
            return super().add_tv_grad(target, scaling, sparse_frac, ignore_edge=ignore_edge)

        def step(self, lr_sigma, lr_sh, beta=0.95, optim="rmsprop"):
            events.append(("step", lr_sigma, lr_sh, beta, optim))
            return super().step(lr_sigma, lr_sh, beta=beta, optim=optim)

        def resample(self, reso, sigma_thresh, weight_thresh, dilate, cameras, max_elements):
            events.append(("resample", list(reso), sigma_thresh, weight_thresh, dilate,
                           None if cameras is None else len(cameras), max_elements))
            return super().resample(reso, sigma_thresh=sigma_thresh, weight_thresh=weight_thresh, dilate=dilate,
                                    cameras=cameras, max_elements=max_elements)

    return Recording


def recording_dataset(base, events):
    class Recording(base):
        def shuffle_rays(self):
            events.append(("shuffle_rays",))
            return super().shuffle_rays()

        def batch(self, begin, end):
            events.append(("batch", begin, end))
            return super().batch(begin, end)

    return Recording


def expected_schedule(cfg, n_rays, n_images):
    """The calls of a run, from opt.py's rules: per epoch a shuffle, then per batch the batch, ``zero_grad``, the fused
    render, the TV terms whose weight is above 0, and the step from ``lr_fg_begin_step`` on; after an epoch that brings the
    steps since the last upsampling to ``upsamp_every``, the TV rule and the resample; the end at ``n_iters``."""
    ev = []
    tv, tv_sh = cfg.lambda_tv, cfg.lambda_tv_sh
    base, last, rid = 0, cfg.init_iters, 0
    while True:
        ev.append(("shuffle_rays",))
        done = 0
        for it, begin in enumerate(range(0, n_rays, cfg.batch_size)):
            g = base + it
            if g >= cfg.n_iters:
                break
            end = min(begin + cfg.batch_size, n_rays)
            ev += [("batch", begin, end), ("zero_grad",)]
            if cfg.lambda_beta or cfg.lambda_sparsity:
                ev.append(("volume_render_fused", end - begin, {"beta_loss": cfg.lambda_beta, "sparsity_loss": cfg.lambda_sparsity}))
            else:
                ev.append(("forward_backward", end - begin, {}))
            if tv > 0:
                ev.append(("add_tv_grad", "density", tv, cfg.tv_sparsity, False))
            if tv_sh > 0:
                ev.append(("add_tv_grad", "sh", tv_sh, cfg.tv_sh_sparsity, True))
            if g >= cfg.lr_fg_begin_step:
                ev.append(("step",
                           expon_lr(g, cfg.lr_sigma, cfg.lr_sigma_final, cfg.lr_sigma_delay_steps, cfg.lr_sigma_delay_mult,
                                    cfg.lr_sigma_decay_steps),
                           expon_lr(g, cfg.lr_sh, cfg.lr_sh_final, cfg.lr_sh_delay_steps, cfg.lr_sh_delay_mult, cfg.lr_sh_decay_steps),
                           cfg.rms_beta, cfg.sigma_optim))
            done = it + 1
        base += done
        if base - last >= cfg.upsamp_every:
            last = base
            if rid < len(cfg.reso) - 1:
                if cfg.tv_early_only > 0:
                    tv = tv_sh = 0.0
                elif cfg.tv_decay != 1.0:
                    tv, tv_sh = tv * cfg.tv_decay, tv_sh * cfg.tv_decay
                rid += 1
                ev.append(("resample", list(cfg.reso[rid]), cfg.density_thresh, cfg.weight_thresh / cfg.reso[rid][2], 2,
                           n_images if cfg.thresh_type == "weight" else None, cfg.max_grid_elements))
        if base >= cfg.n_iters:
            return ev
