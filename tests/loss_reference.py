"""Test-side restatement of the published 3DGS photometric loss (utils/loss_utils.py: gaussian, create_window, _ssim, l1_loss;
train.py: (1 - lambda_dssim) * Ll1 + lambda_dssim * (1 - ssim)), in any dtype.  With dtype=float64 it is the truth the fused
kernels (casualhdrsplat_amd.losses) are held to; with float32 it is the formulation trainers run today ("t32")."""
from math import exp

import torch
import torch.nn.functional as F

WIN, C1, C2 = 11, 0.01 ** 2, 0.03 ** 2


def gaussian_1d(window_size=WIN, sigma=1.5):
    gauss = torch.tensor([exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)],
                         dtype=torch.float32)
    return gauss / gauss.sum()


def window_2d(channels, dtype):
    """create_window: the fp32 outer product of the 1-D window, then cast (the published code's order)."""
    w1 = gaussian_1d().unsqueeze(1)
    w2 = w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0)
    return w2.expand(channels, 1, WIN, WIN).contiguous().to(dtype)


def _as4(t):
    return t.unsqueeze(0) if t.dim() == 3 else t


def ssim_map(x, y, dtype=torch.float64, separable=False, outer_in_dtype=False):
    """_ssim's map for [C,H,W] / [B,C,H,W] inputs.  separable=True runs the window as two 1-D passes; outer_in_dtype=True
    forms the 2-D window's outer product in `dtype` instead of fp32 (what the two passes amount to)."""
    x, y = _as4(x).to(dtype), _as4(y).to(dtype)
    ch = x.shape[1]
    if separable:
        g = gaussian_1d().to(dtype)
        wv = g.view(1, 1, WIN, 1).expand(ch, 1, WIN, 1).contiguous()
        wh = g.view(1, 1, 1, WIN).expand(ch, 1, 1, WIN).contiguous()

        def conv(t):
            t = F.conv2d(t, wh, padding=(0, WIN // 2), groups=ch)
            return F.conv2d(t, wv, padding=(WIN // 2, 0), groups=ch)
    else:
        if outer_in_dtype:
            g = gaussian_1d().to(dtype)
            w = torch.outer(g, g).view(1, 1, WIN, WIN).expand(ch, 1, WIN, WIN).contiguous()
        else:
            w = window_2d(ch, dtype)

        def conv(t):
            return F.conv2d(t, w, padding=WIN // 2, groups=ch)
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = conv(x * x) - mu1_sq
    sigma2_sq = conv(y * y) - mu2_sq
    sigma12 = conv(x * y) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def loss_and_grad(x, y, lambda_dssim, dtype=torch.float64, k=1.0):
    """(loss as a Python float, d(k * loss)/dx as a CPU tensor of `dtype`) by torch autograd on the CPU."""
    xx = x.detach().cpu().to(dtype).requires_grad_(True)
    yy = y.detach().cpu().to(dtype)
    l1 = (xx - yy).abs().mean()
    loss = (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - ssim_map(xx, yy, dtype).mean())
    (k * loss).backward()
    return float(loss.detach()), xx.grad
