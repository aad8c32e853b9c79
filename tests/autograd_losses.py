"""The loss of the autograd fixture (tests/golden/train_autograd.npz): one term on every differentiable output of
render_rays - rgb_map, rgb0, acc_map, acc0, disp_map, disp0 and raw's sigma - with weights that give the terms comparable
size. Shared by the fixture's generator (the reference's autograd) and tests/test_autograd.py (the taped route)."""
import torch


def autograd_loss(ret, target):
    rgb, disp, acc = ret["rgb_map"], ret["disp_map"], ret["acc_map"]
    rgb0, disp0, acc0 = ret["rgb0"], ret["disp0"], ret["acc0"]
    sigma = ret["raw"][..., 3]
    return (torch.mean((rgb - target) ** 2)                       # MSE on rgb (img2mse)
            + 0.5 * torch.mean(torch.abs(rgb0 - target))          # L1 on rgb0
            + 0.5 * torch.mean((acc - 0.75) ** 2)                 # opacity terms
            + 0.1 * torch.mean(acc0)
            + 0.1 * torch.mean(torch.tanh(disp))                  # disparity terms (tanh: a saturated disp is 1e10) ...
            + 0.1 * torch.mean(torch.tanh(2.0 * disp0))
            + 1e-10 * torch.mean(disp + disp0)                    # ... and one whose d/d disp is not 0 there
            + 1e-3 * torch.mean(torch.relu(sigma)))               # a density penalty on raw
