"""Restatement of the transformer's training step for the tests of ``TransformerTrainStep`` (test infrastructure):
forward, loss and gradients of diffusion_transformer.py:82-107 + ``F.mse_loss`` in a chosen dtype with optional
per-site dropout masks, torch's Adam, the EMA recurrence, and the masks themselves built by the existing ``ops.dropout``
on ones (no new code in the yardstick).

The attention is the length-1-sequence identity ``out_proj(v_proj(x))`` that the package runs; with no masks the
restatement is pinned to ``oracle.ref_transformer.train_step_grads`` (which keeps the general softmax formula) by
tests/test_transformer_train_host.py."""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
import torch.nn.functional as F


def forward(p, z, t, y, heads, masks=None):
    """``masks``: None, or 4 L tensors in forward order, each holding 0 or 1 / (1 - p): per block the head mask
    (B, heads) - it scales ``v`` per (row, head), as the module's grouped dropout does - then three (B, D) masks
    (attention output, ff's own dropout, the block's dropout)."""
    dt = z.dtype
    tn = (t / 1000).unsqueeze(-1).float().to(dt)
    h = F.linear(tn, p["time_embedding.0.weight"], p["time_embedding.0.bias"])
    h = h * torch.sigmoid(h)
    emb = F.linear(h, p["time_embedding.2.weight"], p["time_embedding.2.bias"]) + p["class_embedding.weight"][y]
    x = F.linear(z, p["input_proj.weight"], p["input_proj.bias"]) + emb
    x = x + p["pos_encoding"].reshape(-1)
    B, D = x.shape
    i = 0
    while f"transformer_blocks.{i}.norm1.weight" in p:
        pre = f"transformer_blocks.{i}"
        m = None if masks is None else [u.to(dt) for u in masks[4 * i:4 * i + 4]]
        w, b = p[f"{pre}.attention.in_proj_weight"], p[f"{pre}.attention.in_proj_bias"]
        v = F.linear(x, w[2 * D:], b[2 * D:])
        if m is not None:
            v = (v.view(B, heads, D // heads) * m[0].view(B, heads, 1)).reshape(B, D)
        a = F.linear(v, p[f"{pre}.attention.out_proj.weight"], p[f"{pre}.attention.out_proj.bias"])
        if m is not None:
            a = a * m[1]
        x = F.layer_norm(x + a, (D,), p[f"{pre}.norm1.weight"], p[f"{pre}.norm1.bias"])
        f = F.linear(F.gelu(F.linear(x, p[f"{pre}.ff.0.weight"], p[f"{pre}.ff.0.bias"])),
                     p[f"{pre}.ff.2.weight"], p[f"{pre}.ff.2.bias"])
        if m is not None:
            f = f * m[2] * m[3]
        x = F.layer_norm(x + f, (D,), p[f"{pre}.norm2.weight"], p[f"{pre}.norm2.bias"])
        i += 1
    x = F.layer_norm(x, (D,), p["final_layer.0.weight"], p["final_layer.0.bias"])
    return F.linear(x, p["final_layer.1.weight"], p["final_layer.1.bias"])


def loss_of(eps_hat, target, t=None, w_table=None):
    """``F.mse_loss``, or with a (T,) table ``sum_s w[t_s] sum_j (a - b)^2 / n`` (tdx_mse_loss_grad_weighted)."""
    if w_table is None:
        return F.mse_loss(eps_hat, target)
    w = w_table.to(eps_hat.dtype)[t].unsqueeze(-1)
    return (w * (eps_hat - target) ** 2).sum() / eps_hat.numel()


def loss_grads(sd, z_t, t, y, target, heads=4, dtype=torch.float64, masks=None, w_table=None):
    """(loss, eps_hat, OrderedDict of gradients in ``sd``'s order); parameters that take no part (the Q / K thirds
    are slices of one tensor, so this is no whole tensor here) would get zeros."""
    params = OrderedDict((k, v.detach().cpu().to(dtype).clone().requires_grad_(True)) for k, v in sd.items())
    eps = forward(params, z_t.cpu().to(dtype), t.cpu(), y.cpu(), heads, masks)
    loss = loss_of(eps, target.cpu().to(dtype), t.cpu(), None if w_table is None else w_table.cpu())
    grads = torch.autograd.grad(loss, list(params.values()), allow_unused=True)
    grads = [torch.zeros_like(v) if g is None else g for g, v in zip(grads, params.values())]
    return loss.detach(), eps.detach(), OrderedDict(zip(params.keys(), grads))


class Adam:
    """torch.optim.Adam's default single-tensor update on a dict of tensors, in their dtype; ``max_grad_norm``:
    ``clip_grad_norm_`` first.  ``ema_decay``: ``e += (1 - decay_k) (p - e)`` after each update, with the warm-up of
    ``train.ema_decay_at``."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, ema_decay=None,
                 ema_warmup=False):
        self.p = OrderedDict((k, v.detach().clone()) for k, v in params.items())
        self.m = OrderedDict((k, torch.zeros_like(v)) for k, v in self.p.items())
        self.v = OrderedDict((k, torch.zeros_like(v)) for k, v in self.p.items())
        self.lr, self.betas, self.eps, self.max_grad_norm = lr, betas, eps, max_grad_norm
        self.k = 0
        self.ema_decay, self.ema_warmup = ema_decay, ema_warmup
        self.ema = None if ema_decay is None else OrderedDict((k, v.clone()) for k, v in self.p.items())

    def step(self, grads):
        b1, b2 = self.betas
        coef = 1.0
        if self.max_grad_norm is not None:
            norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values()))
            coef = min(1.0, self.max_grad_norm / (norm + 1e-6))
        self.k += 1
        bc1, bc2 = 1.0 - b1 ** self.k, 1.0 - b2 ** self.k
        for k, p in self.p.items():
            g = grads[k].to(p.dtype) * coef
            self.m[k].mul_(b1).add_(g, alpha=1 - b1)
            self.v[k].mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (self.v[k].sqrt() / math.sqrt(bc2)).add_(self.eps)
            p.addcdiv_(self.m[k], denom, value=-self.lr / bc1)
        if self.ema is not None:
            d = self.ema_decay if not self.ema_warmup else min(self.ema_decay, self.k / (9 + self.k))
            for k, e in self.ema.items():
                e.add_((self.p[k] - e) * (1.0 - d))


def train_steps(sd, inputs, heads=4, dtype=torch.float64, lr=1e-3, **adam_kw):
    """``inputs``: per step ``(z_t, t, y, target)``; returns (losses, the Adam object with the final state)."""
    opt = Adam(OrderedDict((k, v.detach().cpu().to(dtype)) for k, v in sd.items()), lr=lr, **adam_kw)
    losses = []
    for z_t, t, y, target in inputs:
        loss, _, g = loss_grads(opt.p, z_t, t, y, target, heads, dtype)
        opt.step(g)
        losses.append(float(loss))
    return losses, opt


def site_masks(seed, offset, B, D, heads, L, p):
    """The 4 L masks that site k = 1 .. 4 L draws from Philox stream ``offset + k`` under key ``seed``: the existing
    ``ops.dropout`` applied to ones (group = head_dim at the head site), as fp64 CPU tensors; None for p == 0."""
    from tiny_diffusion_amd import ops

    if p == 0:
        return None
    ones = torch.ones(B, D, device="cuda")
    out = []
    for l in range(L):
        k = offset + 4 * l
        hm = ops.dropout(ones, p, D // heads, seed, k + 1).view(B, heads, D // heads)
        assert bool((hm == hm[:, :, :1]).all())
        out.append(hm[:, :, 0].double().cpu())
        out += [ops.dropout(ones, p, 1, seed, k + j).double().cpu() for j in (2, 3, 4)]
    return out
