#!/usr/bin/env python3
"""Generate tests/golden/vae_train_B8.npz by running the REFERENCE's own ``VAE`` and ``loss_function`` (vae.py:37-76)
on the CPU: one forward + backward, and three ``torch.optim.Adam(lr=1e-3)`` steps.

Runs only in the build container (needs the reference checkout, like tools/make_golden.py).  The reference's vae.py is
loaded through ``load_reference_latent()`` of tools/make_golden.py and in no other way: that function stubs torchvision
and wandb, so the module body (which builds MNIST datasets with ``download=True``) fetches nothing.

Weights: ``oracle.weights.make_state_dict_vae(0)`` (regenerated on both sides, not stored).  Inputs: one generator
seeded 11 -> x = rand(8, 784) * 2 - 1, then three eps = randn(8, 20); the noise is passed in (the reference's
``reparameterize`` draws its own: vae.py:55-58 is restated with the recorded eps, as make_golden.py does for the latent
fixture).  Stored, per parameter: ``gnorm__<key>`` (double) and ``ghead__<key>`` (first 64 elements) of the one-step
gradient, ``pnorm__`` / ``phead__`` of the parameters after the three steps; the losses.

    python tools/make_golden_vae.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from make_golden import OUT, load_reference_latent  # noqa: E402
from oracle.weights import make_state_dict_vae  # noqa: E402

B, SEED, STEPS, HEAD = 8, 11, 3, 64


def forward_with_eps(vae, x, eps):
    """vae.py:64-67 with the recorded noise in place of torch.randn_like (vae.py:57)."""
    mu, logvar = vae.encode(x.view(-1, vae.config.input_dim))
    z = mu + eps * torch.exp(0.5 * logvar)
    return vae.decode(z), mu, logvar


def main():
    _, vae_mod = load_reference_latent()
    g = torch.Generator().manual_seed(SEED)
    x = torch.rand(B, 784, generator=g) * 2 - 1
    eps = [torch.randn(B, 20, generator=g) for _ in range(STEPS)]
    d = dict(x=x.numpy(), eps=torch.stack(eps).numpy())

    def fresh():
        vae = vae_mod.VAE(vae_mod.VAEConfig())
        vae.load_state_dict(make_state_dict_vae(0), strict=True)
        return vae.train()

    # one step: losses and every parameter gradient
    vae = fresh()
    recon, mu, logvar = forward_with_eps(vae, x, eps[0])
    loss = vae_mod.loss_function(recon, x, mu, logvar)          # vae.py:71-76
    target = (x + 1) / 2
    bce = torch.nn.functional.binary_cross_entropy(recon, target, reduction="sum")
    kld = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())
    loss.backward()
    d.update(loss=np.float64(loss.item()), bce=np.float64(bce.item()), kld=np.float64(kld.item()))
    for k, p in vae.named_parameters():
        gr = p.grad.detach().contiguous().view(-1); kk = k.replace(".", "__")
        d[f"gnorm__{kk}"] = np.float64(gr.double().norm().item())
        d[f"ghead__{kk}"] = gr[:HEAD].numpy().copy()
    # three Adam steps on the same x (vae.py:97, 110-115)
    vae = fresh()
    opt = torch.optim.Adam(vae.parameters(), lr=1e-3)
    losses = []
    for e in eps:
        opt.zero_grad()
        recon, mu, logvar = forward_with_eps(vae, x, e)
        loss = vae_mod.loss_function(recon, x, mu, logvar)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    d["adam_losses"] = np.asarray(losses, np.float64)
    for k, p in vae.named_parameters():
        v = p.detach().contiguous().view(-1); kk = k.replace(".", "__")
        d[f"pnorm__{kk}"] = np.float64(v.double().norm().item())
        d[f"phead__{kk}"] = v[:HEAD].numpy().copy()
    assert list(dict(vae.named_parameters())) == list(make_state_dict_vae(0))
    path = os.path.join(OUT, "vae_train_B8.npz")
    np.savez_compressed(path, **d)
    print(f"vae_train_B8: loss {d['loss']:.6f} = bce {d['bce']:.6f} + kld {d['kld']:.6f}; adam {losses}; "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
