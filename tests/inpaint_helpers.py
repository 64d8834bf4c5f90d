"""Helpers of the inpainting tests (tests/test_inpaint_host.py, tests/test_gpu_inpaint.py): the fp32 restatements of the
masked updates (every product and sum a separate torch op, in the kernels' order), the fp64 chains with the blend, masks
of 0 / 1 / fractional blocks, and the models / inputs / fp64 networks the chain tests share.  Restated here, not
imported from a test module."""
import math

import torch

INF = float("inf")
NUM_CLASSES = 10
SHAPES = {"uncond": (1, 28, 28), "cond": (1, 28, 28), "laion": (4, 32, 32), "latent": (20,), "transformer": (20,)}


# ---------------------------------------------------------------- the blend and the x0-form updates, fp32 on the CPU
def blend32(x0c, known, m):
    """x0_blend of csrc/common.h: (1 - m) * x0c + m * known, each operation rounded separately in fp32."""
    one = torch.tensor(1.0, dtype=torch.float32)
    return (one - m) * x0c + m * known


def cfg32(oc, ou, w):
    return ou + torch.tensor(w, dtype=torch.float32) * (oc - ou)


def clamp32(x0, lo, hi):
    return torch.minimum(torch.maximum(x0, torch.tensor(lo)), torch.tensor(hi))


def cpu_x0_step(x, out, z, row, lo, hi, k, w=None):
    """The x0-form update (pstep_elem, TDX_STEP_X0), every product and sum a separate torch op in the kernel's order:
    returns (x', x0)."""
    p, q, A, Bx, sg = row.unbind()
    if w is not None:
        n = x.shape[0]
        out = cfg32(out[:n], out[n:], w)
    x0 = p * x + q * out
    zz = z if (z is not None and k > 0) else torch.zeros_like(x)
    return (A * clamp32(x0, lo, hi) + Bx * x) + sg * zz, x0


def cpu_ms_step(x, out, hist, row, lo, hi):
    """The multistep update (pstep_elem, TDX_STEP_MS) likewise; the H term only when H != 0.  Returns (x', the clamped
    x0, x0)."""
    p, q, A, Bx, H = row.unbind()
    x0 = p * x + q * out
    x0c = clamp32(x0, lo, hi)
    r = A * x0c + Bx * x
    if H.item() != 0.0:
        r = r + H * hist
    return r, x0c, x0


def cpu_x0_masked_step(x, out, z, known, m, row, lo, hi, k, w=None):
    """cpu_x0_step with the blend between the clamp and the step: returns (x', x0, x0m)."""
    p, q, A, Bx, sg = row.unbind()
    if w is not None:
        n = x.shape[0]
        out = cfg32(out[:n], out[n:], w)
    x0 = p * x + q * out
    x0m = blend32(clamp32(x0, lo, hi), known, m)
    zz = z if (z is not None and k > 0) else torch.zeros_like(x)
    return (A * x0m + Bx * x) + sg * zz, x0, x0m


def cpu_ms_masked_step(x, out, hist, known, m, row, lo, hi, w=None):
    """cpu_ms_step with the blend: returns (x', x0, x0m); the history term only at H != 0."""
    p, q, A, Bx, H = row.unbind()
    if w is not None:
        n = x.shape[0]
        out = cfg32(out[:n], out[n:], w)
    x0 = p * x + q * out
    x0m = blend32(clamp32(x0, lo, hi), known, m)
    r = A * x0m + Bx * x
    if H.item() != 0.0:
        r = r + H * hist
    return r, x0, x0m


# ---------------------------------------------------------------- which update a sampler asked for
def spy_entries(monkeypatch, lib, names, calls):
    """Append the name of every call of the C entries ``names`` to ``calls``.  The two entries that take every update
    are recorded with the update the call asks for - its form, ``sched`` under a timestep schedule, ``guided``,
    ``masked`` - as in ``tdx_p_sample_update[x0,sched,guided,masked]``."""
    where = {"tdx_p_sample_update": (4, 7, 11, 16), "tdx_unet_eval_step_update": (18, 7, 19, 24)}   # form, tau, guided, known

    def spy(real, name):
        def call(*a):
            tag = name
            if name in where:
                f, t, g, k = where[name]
                tag += "[" + ",".join([("eps", "x0", "ms")[a[f]]] + ["sched"] * (a[t] is not None) + ["guided"] * bool(a[g])
                                      + ["masked"] * (a[k] is not None)) + "]"
            calls.append(tag)
            return real(*a)
        return call
    for name in names:
        monkeypatch.setattr(lib, name, spy(getattr(lib, name), name))


# ---------------------------------------------------------------- masks and known data
def block_mask(shape, binary=False):
    """A mask of shape (1, 1, H, W) / (1, D) that broadcasts over samples (and channels): a block of exact 1, a block of
    fractions (0.25 and 0.5; exact 1 in their place when ``binary``) and the rest exact 0."""
    frac = (1.0, 1.0) if binary else (0.25, 0.5)
    if len(shape) == 3:
        _, H, W = shape
        m = torch.zeros(1, 1, H, W)
        m[..., : H // 2, : W // 2] = 1.0
        m[..., : H // 2, W // 2: W // 2 + 3] = frac[0]
        m[..., H // 2: H // 2 + 3, : W // 2] = frac[1]
    else:
        D = shape[0]
        m = torch.zeros(1, D)
        m[:, : D // 3] = 1.0
        m[:, D // 3: D // 3 + 2] = frac[0]
        m[:, D // 3 + 2: D // 3 + 4] = frac[1]
    return m


def known_data(n, shape, seed=0):
    """Finite data, some of it outside [-1, 1] (known is the user's: it is not clamped)."""
    g = torch.Generator().manual_seed(1000 + seed)
    return (1.2 * (2 * torch.rand(n, *shape, generator=g) - 1)).contiguous()


# ---------------------------------------------------------------- models, inputs, the oracle's networks in double
def model(kind, seed=0):
    from oracle.weights import (make_state_dict, make_state_dict_laion, make_state_dict_latent,
                                make_state_dict_transformer)
    if kind == "uncond":
        from tiny_diffusion_amd.diffusion import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict(seed, False), strict=True)
    elif kind == "cond":
        from tiny_diffusion_amd.conditional_diffusion import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict(seed, True), strict=True)
    elif kind == "laion":
        from tiny_diffusion_amd.conditional_diffusion_laion import NoiseModel
        m = NoiseModel(time_dim=768)
        m.load_state_dict(make_state_dict_laion(seed), strict=True)
    elif kind == "latent":
        from tiny_diffusion_amd.latent_diffusion import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict_latent(seed), strict=True)
    else:
        from tiny_diffusion_amd.diffusion_transformer import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict_transformer(seed), strict=True)
    return m.cuda()


def inputs(kind, n, T, seed=0):
    """(x_T, T recorded noises, condition on the GPU)."""
    g = torch.Generator().manual_seed(seed)
    x_T = torch.randn(n, *SHAPES[kind], generator=g)
    zs = torch.randn(T, n, *SHAPES[kind], generator=g)
    if kind == "uncond":
        y = None
    elif kind == "laion":
        y = torch.randn(n, 768, generator=g).cuda()
    else:
        y = torch.randint(0, NUM_CLASSES, (n,), generator=g).cuda()
    return x_T, zs, y


def null_cond(kind, y):
    return torch.zeros_like(y) if kind == "laion" else torch.full_like(y, -1)


def amp(w):
    """How out_u + w (out_c - out_u) amplifies an error in either output (squared: the tolerances are mean squares)."""
    return 1.0 if w is None else (abs(w) + abs(w - 1.0)) ** 2


def fp64_forward(kind, seed):
    """out(x, t, y) of the oracle's network in double; for the conditional MNIST UNet a label -1 is the null condition
    (one zero row appended to this copy of class_embedding.weight)."""
    from oracle import ref_cpu as R
    from oracle import ref_laion as RLA
    from oracle import ref_latent as RLT
    from oracle import ref_transformer as RT
    from oracle.weights import (make_state_dict, make_state_dict_laion, make_state_dict_latent,
                                make_state_dict_transformer)
    if kind in ("uncond", "cond", "laion"):
        sd = make_state_dict_laion(seed) if kind == "laion" else make_state_dict(seed, kind == "cond")
        if kind == "cond":
            w = sd["class_embedding.weight"]
            sd["class_embedding.weight"] = torch.cat([w, torch.zeros(1, w.shape[1], dtype=w.dtype)])
        p, b = R.split_state(sd)
    elif kind == "latent":
        p, b = R.split_state(make_state_dict_latent(seed))
    else:
        p, b = dict(make_state_dict_transformer(seed)), {}
    p = {k: v.double() for k, v in p.items()}
    b = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in b.items()}

    def fwd(x, t, y):
        yy = None if y is None else y.cpu()
        if kind == "laion":
            return RLA.unet_forward(p, b, x, t, yy.double(), training=False)
        if kind == "latent":
            return RLT.noise_forward(p, b, x, t, yy, training=False)
        if kind == "transformer":
            return RT.noise_forward(p, x, t, yy)
        if kind == "cond":
            yy = torch.where(yy < 0, torch.full_like(yy, NUM_CLASSES), yy)
        return R.unet_forward(p, b, x, t, yy, training=False)
    return fwd


# ---------------------------------------------------------------- the fp64 chains with the blend
def _out64(fwd, kind, x, t, y, w):
    if w is None:
        return fwd(x, t, y)
    n = x.shape[0]
    o = fwd(torch.cat([x, x]), torch.cat([t, t]), torch.cat([y, null_cond(kind, y)]))
    return o[n:] + w * (o[:n] - o[n:])


def x0_rows64(fp, sched):
    """(a, b, A, Bx, sigma) per step in Python doubles, from this file's own expressions: DDIM rows from Song et al.'s
    closed forms on the fp64 ``alphas_cumprod``, DDPM rows from the reference's fp32 (c1, c2, sigma) (its chain is
    defined by them) through A = c1 c2 a / b, Bx = c1 (b - c2) / b.  Row 0: A = 1, Bx = 0."""
    acp = fp.alphas_cumprod.double()
    taus = sched.timesteps.tolist()
    rows = []
    for k, t in enumerate(taus):
        ab = acp[t].item()
        a, b = math.sqrt(ab), math.sqrt(1 - ab)
        if sched.eta is None:
            c1, c2, sg = fp.tables("cpu")[2][t].double().tolist()
            A, Bx = c1 * c2 * a / b, c1 * (b - c2) / b
        else:
            ab_prev = acp[taus[k - 1]].item() if k > 0 else 1.0
            sg = sched.eta * math.sqrt((1 - ab_prev) / (1 - ab)) * math.sqrt(1 - ab / ab_prev)
            r = math.sqrt(1 - ab_prev - sg * sg)
            A, Bx = math.sqrt(ab_prev) - a * r / b, r / b
        rows.append((a, b, 1.0, 0.0, sg) if k == 0 else (a, b, A, Bx, sg))
    return rows


@torch.no_grad()
def inpaint_chain64(fwd, kind, fp, sched, x_T, y, known, mask, lo=-INF, hi=INF, prediction="eps", w=None, zs=None):
    """The x0-form chain with the blend, fp64 state:  x0 = (x - b out) / a (eps) or a x - b out (v);  x0c = clamp(x0);
    x0m = (1 - mask) x0c + mask known;  x' = A x0m + Bx x + sigma z."""
    x = x_T.double()
    known, mask = known.double(), mask.double()
    n = x.shape[0]
    taus = sched.timesteps.tolist()
    for k, (a, b, A, Bx, sg) in reversed(list(enumerate(x0_rows64(fp, sched)))):
        t = torch.full((n,), taus[k], dtype=torch.long)
        out = _out64(fwd, kind, x, t, y, w)
        x0 = (x - b * out) / a if prediction == "eps" else a * x - b * out
        x0m = (1 - mask) * torch.clamp(x0, lo, hi) + mask * known
        x = A * x0m + Bx * x
        if k > 0 and sg > 0:
            x = x + sg * zs[taus[k]].double()
    return x


@torch.no_grad()
def inpaint_dpm_chain64(fwd, kind, fp, taus, x_T, y, known, mask, lo=-INF, hi=INF, prediction="eps", w=None, order=2):
    """DPM-Solver++(2M) from its closed forms in Python doubles, with the blend: D is built from the BLENDED predictions
    x0m of this step and the step before;  x' = (b'/b) x + a' (1 - e^{-h}) D;  the last step returns x0m."""
    acp = fp.alphas_cumprod.double()
    ab = [(math.sqrt(acp[t].item()), math.sqrt(1 - acp[t].item())) for t in taus]
    lam = [math.log(a / b) for a, b in ab]
    x = x_T.double()
    known, mask = known.double(), mask.double()
    n, S = x.shape[0], len(taus)
    prev = None
    for k in range(S - 1, -1, -1):
        a, b = ab[k]
        t = torch.full((n,), taus[k], dtype=torch.long)
        out = _out64(fwd, kind, x, t, y, w)
        x0 = (x - b * out) / a if prediction == "eps" else a * x - b * out
        x0m = (1 - mask) * torch.clamp(x0, lo, hi) + mask * known
        if k == 0:
            return x0m
        a1, b1 = ab[k - 1]
        h = lam[k - 1] - lam[k]
        D = x0m
        if order == 2 and k < S - 1:
            r = (lam[k] - lam[k + 1]) / h
            D = (1 + 1 / (2 * r)) * x0m - (1 / (2 * r)) * prev
        x = (b1 / b) * x + a1 * -math.expm1(-h) * D
        prev = x0m
