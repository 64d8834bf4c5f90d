#!/usr/bin/env python3
"""Generate tests/golden/transformer_train_B16.npz by running the REFERENCE's own ``NoiseModel(dropout=0.0)``
(diffusion_transformer.py:38-107) in train mode on the CPU: three ``torch.optim.Adam(lr=1e-3)`` steps of
``F.mse_loss(model(z_t, t, y), noise)`` (diffusion_transformer.py:197-202).

Runs only in the build container (needs the reference checkout, like tools/make_golden.py).  The reference module is
loaded the way ``transformer_fixtures()`` of tools/make_golden.py loads it: ``load_reference_latent()`` registers the
torchvision / wandb / vae stubs first, so the import fetches nothing.

Weights: ``oracle.weights.make_state_dict_transformer(0)`` (regenerated on both sides, not stored).  Inputs: ``z_t, t,
y, noise`` of tests/golden/transformer_B16.npz; step k uses ``z_t + 0.1 * pert[k]`` with ``pert = randn(3, 16, 20)``
from a generator seeded 23 (recorded).  Stored: the three losses; per parameter ``gnorm__<key>`` (double, the gradient
norm of step 1) and ``phead__<key>`` (the first 64 elements after step 3).

    python tools/make_golden_transformer_train.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from make_golden import OUT, REF, load_reference_latent  # noqa: E402
from oracle.weights import make_state_dict_transformer  # noqa: E402

SEED, STEPS, HEAD, LR, PERT = 23, 3, 64, 1e-3, 0.1


def main():
    load_reference_latent()   # registers the torchvision / wandb / vae stubs
    spec = importlib.util.spec_from_file_location("ref_diffusion_transformer",
                                                  os.path.join(REF, "diffusion_transformer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    src = np.load(os.path.join(OUT, "transformer_B16.npz"))
    z_t, t, y, noise = (torch.from_numpy(src[k]) for k in ("z_t", "t", "y", "noise"))
    pert = torch.randn(STEPS, *z_t.shape, generator=torch.Generator().manual_seed(SEED))
    d = dict(pert=pert.numpy(), pert_scale=np.float64(PERT), lr=np.float64(LR))
    sd = make_state_dict_transformer(0)
    model = mod.NoiseModel(dropout=0.0)
    model.load_state_dict(sd, strict=True)
    model.train()
    assert list(dict(model.named_parameters())) == list(sd)
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    losses = []
    for k in range(STEPS):
        loss = F.mse_loss(model(z_t + PERT * pert[k], t, y), noise)
        opt.zero_grad()
        loss.backward()
        if k == 0:
            for name, p in model.named_parameters():
                d["gnorm__" + name.replace(".", "__")] = np.float64(p.grad.double().norm().item())
        opt.step()
        losses.append(loss.item())
    d["losses"] = np.asarray(losses, np.float64)
    for name, p in model.named_parameters():
        d["phead__" + name.replace(".", "__")] = p.detach().contiguous().view(-1)[:HEAD].numpy().copy()
    path = os.path.join(OUT, "transformer_train_B16.npz")
    np.savez_compressed(path, **d)
    print(f"transformer_train_B16: losses {losses}; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
