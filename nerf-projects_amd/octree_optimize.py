"""Fine-tuning a PlenOctree on images: the loop of ``plenoctree/octree/optimization.py`` on :class:`octree.N3Tree`.

Per training image the reference renders with ``render_persp``, clamps, takes the MSE, calls ``mse.backward()`` and steps
``SGD(t.parameters(), lr=1e7)``; here those are one launch (:meth:`N3Tree.mse_backward`) and the optimizer's step. Images stay
on the device, and nothing waits for it except the PSNR reads at a validation."""
import numpy as np
import torch

from .grid import Camera

__all__ = ["optimize", "optimize_blender", "psnr_of"]


def psnr_of(mse):
    """``-10 log10(mse)`` of a tensor, on its device."""
    return -10.0 * torch.log10(mse)


def _validate(tree, cameras, images, options):
    """Mean PSNR of the clamped renders over the validation views (one wait, for the read)."""
    with torch.no_grad():
        total = torch.zeros((), device=tree.device)
        for cam, gt in zip(cameras, images):
            im = tree.volume_render_image(cam, **options).clamp_(0.0, 1.0)
            total = total + psnr_of(((im - gt) ** 2).mean())
    return float(total) / max(len(cameras), 1)


def optimize(tree, train_cameras, train_images, val_cameras, val_images, num_epochs=80, lr=1e7, sgd=True, sgd_momentum=0.0,
             sgd_nesterov=False, val_interval=2, continue_on_decrease=False, **options):
    """``optimization.py``'s loop: an initial validation; per epoch, for every training image, the fused clamped-MSE backward
    and an optimizer step (``SGD(lr, momentum, nesterov)``, or ``Adam(lr, eps=1e-8)`` with ``sgd=False``), and the mean train
    PSNR; a validation every ``val_interval`` epochs and after the last, which keeps a clone of the tree where the PSNR rose
    and otherwise ends the loop unless ``continue_on_decrease``. ``tree`` is updated in place (its ``data`` is made to require
    grad); ``*_cameras`` are :class:`grid.Camera`, ``*_images`` ``[H, W, 3]`` tensors, moved to the tree's device once;
    ``options`` are the render options of :meth:`N3Tree.volume_render_image`.
    Returns ``(best, history)``: ``best`` is the clone with the best validation PSNR, or ``None`` where no validation beat
    the initial one; ``history = {"initial_val_psnr", "train_psnr": [per epoch], "val_psnr": [(epoch, psnr), ...],
    "best_val_psnr"}``."""
    if len(train_cameras) != len(train_images) or len(val_cameras) != len(val_images):
        raise ValueError("one image per camera is required")
    if val_interval < 1:
        raise ValueError(f"val_interval = {val_interval} must be at least 1")
    dev = tree.device
    train_images = [torch.as_tensor(im, dtype=torch.float32).to(dev) for im in train_images]
    val_images = [torch.as_tensor(im, dtype=torch.float32).to(dev) for im in val_images]
    tree.requires_grad_(True)
    if sgd:
        optimizer = torch.optim.SGD(tree.parameters(), lr=lr, momentum=sgd_momentum, nesterov=sgd_nesterov)
    else:
        optimizer = torch.optim.Adam(tree.parameters(), lr=lr, eps=1e-8)
    best_psnr = _validate(tree, val_cameras, val_images, options)
    history = {"initial_val_psnr": best_psnr, "train_psnr": [], "val_psnr": [], "best_val_psnr": best_psnr}
    best = None
    pending = []      # the epochs' train PSNR, still on the device
    for epoch in range(num_epochs):
        total = torch.zeros((), device=dev)
        for cam, gt in zip(train_cameras, train_images):
            optimizer.zero_grad(set_to_none=False)      # (the gradient array is kept and zeroed: mse_backward adds into it)
            mse = tree.mse_backward(cam, gt, **options)
            optimizer.step()
            total = total + psnr_of(mse)
        pending.append(total / max(len(train_cameras), 1))
        if epoch % val_interval == val_interval - 1 or epoch == num_epochs - 1:
            val = _validate(tree, val_cameras, val_images, options)
            history["val_psnr"].append((epoch, val))
            history["train_psnr"] += [float(p) for p in pending]
            pending = []
            if val > best_psnr:
                best_psnr = history["best_val_psnr"] = val
                best = tree.clone()
            elif not continue_on_decrease:
                break
    history["train_psnr"] += [float(p) for p in pending]
    return best, history


def optimize_blender(tree, basedir, half_res=False, testskip=1, **kw):
    """:func:`optimize` on a NeRF-synthetic scene directory: ``datasets.load_blender_data``'s train and val splits, alpha
    composited on white, one ``Camera.from_nerf_pose`` per frame."""
    from . import datasets
    imgs, poses, _, (H, W, focal), (i_train, i_val, _) = datasets.load_blender_data(basedir, half_res=half_res, testskip=testskip)
    imgs = np.asarray(imgs, dtype=np.float32)
    if imgs.shape[-1] == 4:
        imgs = imgs[..., :3] * imgs[..., 3:] + (1.0 - imgs[..., 3:])
    cams = [Camera.from_nerf_pose(p, int(H), int(W), float(focal)) for p in poses]
    pick = lambda idx: ([cams[i] for i in idx], [torch.from_numpy(np.ascontiguousarray(imgs[i])) for i in idx])      # noqa: E731
    tc, ti = pick(i_train)
    vc, vi = pick(i_val)
    return optimize(tree, tc, ti, vc, vi, **kw)
