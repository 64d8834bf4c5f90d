"""A functional torch restatement of the VAE's training step (vae.py:51-76, 110-115): forward with supplied noise, the
sum-reduced BCE + KLD loss and the autograd gradients, in fp32 or fp64, on the CPU.  Shared by the VAE training tests;
a plain module, not a conftest.

``form="sigmoid"`` is the reference's arithmetic (``F.binary_cross_entropy(torch.sigmoid(a), target)``), ``form="logits"``
the kernel's (``max(a, 0) - a t + log1p(exp(-|a|))``); in fp64 the two agree to 1e-12 wherever torch's clamp
``log >= -100`` does not bind."""
import numpy as np
import torch
import torch.nn.functional as F

KEYS = ("fc1.weight", "fc1.bias", "fc21.weight", "fc21.bias", "fc22.weight", "fc22.bias", "fc3.weight", "fc3.bias",
        "fc4.weight", "fc4.bias")


def recipe_inputs(seed, B, input_dim=784, latent_dim=20, n_eps=1):
    """The fixture's input recipe: x uniform in [-1, 1), then ``n_eps`` standard-normal eps, from one generator."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, input_dim, generator=g) * 2 - 1
    eps = [torch.randn(B, latent_dim, generator=g) for _ in range(n_eps)]
    return x, (eps[0] if n_eps == 1 else eps)


def default_init_state_dict(seed, input_dim, hidden_dim, latent_dim):
    """nn.Linear's default initialisation in the reference's construction order (fc1, fc21, fc22, fc3, fc4)."""
    torch.manual_seed(seed)
    shapes = (("fc1", input_dim, hidden_dim), ("fc21", hidden_dim, latent_dim), ("fc22", hidden_dim, latent_dim),
              ("fc3", latent_dim, hidden_dim), ("fc4", hidden_dim, input_dim))
    sd = {}
    for name, cin, cout in shapes:
        lin = torch.nn.Linear(cin, cout)
        sd[name + ".weight"], sd[name + ".bias"] = lin.weight.detach().clone(), lin.bias.detach().clone()
    return sd


def bce_sum(a, target, form):
    if form == "sigmoid":
        return F.binary_cross_entropy(torch.sigmoid(a), target, reduction="sum")
    return (a.clamp(min=0) - a * target + torch.log1p(torch.exp(-a.abs()))).sum()


def forward_loss(p, x, eps, kld_weight=1.0, form="sigmoid"):
    """(loss, bce, kld, aux) from a dict of parameter tensors ``p``; aux: pre-activations of the two ReLU layers, the
    logits, mu and logvar (what the tests' input conditions are stated on)."""
    x = x.reshape(x.shape[0], -1)
    pre1 = F.linear(x, p["fc1.weight"], p["fc1.bias"])
    h1 = F.relu(pre1)
    mu = F.linear(h1, p["fc21.weight"], p["fc21.bias"])
    logvar = F.linear(h1, p["fc22.weight"], p["fc22.bias"])
    z = mu + eps * torch.exp(0.5 * logvar)
    pre3 = F.linear(z, p["fc3.weight"], p["fc3.bias"])
    a = F.linear(F.relu(pre3), p["fc4.weight"], p["fc4.bias"])
    bce = bce_sum(a, (x + 1) / 2, form)
    kld = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())
    return bce + kld_weight * kld, bce, kld, dict(pre1=pre1, pre3=pre3, logits=a, mu=mu, logvar=logvar)


def loss_and_grads(sd, x, eps, kld_weight=1.0, dtype=torch.float32, form="sigmoid"):
    """One forward + backward.  Returns dict(loss, bce, kld: Python floats; grads: {key: tensor}; aux)."""
    p = {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in KEYS}
    loss, bce, kld, aux = forward_loss(p, x.to(dtype), eps.to(dtype), kld_weight, form)
    grads = torch.autograd.grad(loss, [p[k] for k in KEYS])
    return dict(loss=loss.item(), bce=bce.item(), kld=kld.item(), grads=dict(zip(KEYS, (g.detach() for g in grads))),
                aux={k: v.detach() for k, v in aux.items()})


def input_margins(aux):
    """(smallest |pre-activation| over both ReLU layers, largest |logit|, largest |logvar|)."""
    return (min(aux["pre1"].abs().min().item(), aux["pre3"].abs().min().item()), aux["logits"].abs().max().item(),
            aux["logvar"].abs().max().item())


def adam_steps(sd, x, eps_list, lr=1e-3, kld_weight=1.0, dtype=torch.float32, form="sigmoid", max_grad_norm=None):
    """len(eps_list) steps of torch.optim.Adam(lr) on the same ``x``.  Returns (losses, final parameters)."""
    p = {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in KEYS}
    opt = torch.optim.Adam([p[k] for k in KEYS], lr=lr)
    losses = []
    for eps in eps_list:
        opt.zero_grad()
        loss = forward_loss(p, x.to(dtype), eps.to(dtype), kld_weight, form)[0]
        loss.backward()
        if max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_([p[k] for k in KEYS], max_grad_norm)
        opt.step()
        losses.append(loss.item())
    return losses, {k: v.detach() for k, v in p.items()}


def rel_l2(got, want):
    got, want = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1)
    return (got - want).norm().item() / max(want.norm().item(), 1e-300)


def rel_err(got, want):
    return abs(float(got) - float(want)) / max(abs(float(want)), 1e-300)


def head_tolerance(gnorm, numel, rtol=1e-4, atol_scale=1e-5):
    """(rtol, atol) of the ``ghead`` comparison: atol = 1e-5 * gnorm / sqrt(numel), the gradient's RMS scaled."""
    return rtol, atol_scale * float(gnorm) / np.sqrt(numel)
