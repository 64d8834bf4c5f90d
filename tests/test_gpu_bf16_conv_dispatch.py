"""The bf16 MFMA convolution kernels of csrc/conv3x3_bf16.hip per element, at every branch of their dispatch
(DESIGN.md 3.26): the 128-row, ring and thin forward / input-gradient kernels, the per-tap, swizzled per-tap and
nine-tap weight-gradient kernels, and the pack - through the C entries, as tests/test_gpu_bf16.py calls them, whose
norm-wise gates stay where they are.

Cases, operands, references, gates and the kernel each case reaches: tests/bf16_conv_helpers.py, checked on the CPU
by tests/test_bf16_conv_refs_host.py.  Every case runs in two regimes.  exact: small-integer operands, every fp32
accumulation exact in any order - fp32 outputs torch.equal the fp64 reference, bf16 outputs equal its nearest-even
rounding, no tolerance (M2 alone: LAM u sqrt(rows) M2).  rounding: |got - ref| <= 9 u sqrt(K) x magnitude-sum for fp32
outputs, the interval [RNE(ref - b), RNE(ref + b)] for bf16 ones.  Every output starts as NaN behind CH.Guards; knobs
are set with tdx.tuned only.  `-s` prints the worst figure per launch family."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16_conv_helpers as BC  # noqa: E402
import conv_helpers as CH  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
WORST = {}


@pytest.fixture(scope="module")
def tdx():
    import tiny_diffusion_amd._lib as L

    assert torch.cuda.is_available()
    return L


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(t, io16=0):
    if t is None:
        return None
    return (t.to(BF16) if io16 else t).contiguous().cuda()


def note(family, regime, fig):
    key = (family, regime)
    WORST[key] = max(WORST.get(key, 0.0), float(fig))


def packs(tdx, d, cout, cin):
    wf = torch.full((cout * 9 * cin,), float("nan"), dtype=BF16, device="cuda")
    wg = torch.full((cout * 9 * cin,), float("nan"), dtype=BF16, device="cuda")
    tdx.check(tdx.lib.tdx_pack_conv3x3_bf16(dev(d["w"]).data_ptr(), wf.data_ptr(), wg.data_ptr(), cout, cin, st()))
    return wf, wg


def run_fwd(tdx, guards, shape, x, wpk, bias, flags, io16, isc=None, ish=None, osc=None, osh=None):
    """One tdx_conv3x3_fwd_bf16_io launch on guarded NaN outputs -> (out, stats or None)."""
    B, Hh, W, cin, cout = shape
    out = guards.new((B, Hh, W, cout), BF16 if io16 else F32)
    stats = guards.new((-(-B * Hh * W // BC.STAT_ROWS), 2, cout)) if flags & BC.FLAG_STATS else None
    tdx.check(tdx.lib.tdx_conv3x3_fwd_bf16_io(x.data_ptr(), wpk.data_ptr(), CH.p(bias), out.data_ptr(), B, Hh, W, cin, cout,
                                              flags, CH.p(isc), CH.p(ish), CH.p(osc), CH.p(osh), CH.p(stats), io16, st()))
    return out, stats


@pytest.mark.parametrize("regime", BC.REGIMES)
@pytest.mark.parametrize("name", list(BC.FWD_CASES))
def test_forward_and_input_gradient_per_element(tdx, name, regime):
    shape, knobs, io16s, in_bns, family = BC.FWD_CASES[name]
    B, Hh, W, cin, cout = shape
    d = BC.operands(shape, regime)
    guards = CH.Guards()
    fails = []
    with tdx.tuned(**knobs):
        wf, wg = packs(tdx, d, cout, cin)
        bias, isc, ish, osc, osh = (dev(d[k]) for k in ("b", "isc", "ish", "osc", "osh"))
        for io16 in io16s:
            x, dy = dev(d["x"], io16), dev(d["dy"], io16)
            for in_bn in in_bns:
                r = BC.fwd_refs(shape, regime, in_bn)
                bn = (isc, ish) if in_bn else (None, None)
                tag = f"{name} io16={io16} in_bn={in_bn}"
                fam = f"{family} fwd {'bf16' if io16 else 'fp32'}"
                plain, _ = run_fwd(tdx, guards, shape, x, wf, bias, in_bn, io16, *bn)
                train, stats = run_fwd(tdx, guards, shape, x, wf, bias, in_bn | BC.FLAG_STATS, io16, *bn)
                infer, _ = run_fwd(tdx, guards, shape, x, wf, bias, in_bn | BC.FLAG_INFER, io16, *bn, osc, osh)
                torch.cuda.synchronize()
                for what, got in (("plain", plain), ("stats-launch", train)):
                    ok, fig = BC.held(got, regime, r["ref"], r["b"], r["mag"], r["K"])
                    note(fam, regime, fig)
                    print(f"{tag} {what}: {fig:.3g}")
                    if not ok:
                        fails.append(f"{tag} {what}: {fig:.3g}")
                ok, fig = BC.held(infer, regime, r["pre"], r["b_inf"], r["mag_inf"], r["K"], relu=True)
                note(fam + " infer", regime, fig)
                print(f"{tag} infer: {fig:.3g}")
                if not ok:
                    fails.append(f"{tag} infer: {fig:.3g}")
                ok, fs, fm = BC.stats_held(stats, r["stats"], regime)
                note(f"{family} stats sum", regime, fs)
                note(f"{family} stats M2", regime, fm)
                print(f"{tag} stats: sum {fs:.3g} M2 {fm:.3g}")
                if not ok:
                    fails.append(f"{tag} statistics: sum {fs:.3g} M2 {fm:.3g}")
            # input gradient: the plain launch on dy with the mirrored pack, channel roles swapped
            g = BC.dgrad_refs(shape, regime)
            gin, _ = run_fwd(tdx, guards, (B, Hh, W, cout, cin), dy, wg, None, 0, io16)
            torch.cuda.synchronize()
            ok, fig = BC.held(gin, regime, g["ref"], g["b"], g["mag"], g["K"])
            note(f"dgrad {'bf16' if io16 else 'fp32'}", regime, fig)
            print(f"{name} io16={io16} dgrad: {fig:.3g}")
            if not ok:
                fails.append(f"{name} io16={io16} dgrad: {fig:.3g}")
            if name == "ring-cin1088":   # past the ring's gate the knob changes nothing: bit-equal to bf16_ring = 0
                for in_bn in in_bns:
                    bn = (isc, ish) if in_bn else (None, None)
                    here, _ = run_fwd(tdx, guards, shape, x, wf, bias, in_bn, io16, *bn)
                    with tdx.tuned(**BC.RING_TWIN):
                        twin, _ = run_fwd(tdx, guards, shape, x, wf, bias, in_bn, io16, *bn)
                    torch.cuda.synchronize()
                    if not torch.equal(here, twin):
                        fails.append(f"ring-cin1088 in_bn={in_bn} differs from the 128-row kernel's result")
        if not guards.intact():
            fails.append("guard region written")
    print({k: v for k, v in WORST.items() if k[1] == regime})
    assert not fails, fails


def _wgrad_id(run):
    shape, io16, kn = run
    return "x".join(map(str, shape)) + f"-io{io16}-{kn}"


@pytest.mark.parametrize("regime", BC.REGIMES)
@pytest.mark.parametrize("run", BC.wgrad_runs(), ids=_wgrad_id)
def test_weight_gradient_per_element(tdx, run, regime):
    shape, io16, kn = run
    B, Hh, W, cin, cout = shape
    knobs = BC.WGRAD_KNOBS[kn]
    d = BC.operands(shape, regime)
    guards = CH.Guards()
    fails = []
    x, dy, isc, ish = dev(d["x"], io16), dev(d["dy"], io16), dev(d["isc"]), dev(d["ish"])
    with tdx.tuned(**knobs):
        splits = tdx.lib.tdx_conv3x3_wgrad_splits_bf16(B, Hh, W, cin, cout)
        assert splits == BC.wgrad_plan(B * Hh * W, cin, cout, knobs)[2]
        for in_bn in (0, 1):
            r = BC.wgrad_refs(shape, regime, in_bn)
            slabs = guards.new((splits, cout, 9, cin))
            dw = guards.new((cout, cin, 3, 3))
            tdx.check(tdx.lib.tdx_conv3x3_wgrad_bf16_io(x.data_ptr(), dy.data_ptr(), slabs.data_ptr(), B, Hh, W, cin, cout,
                                                        in_bn, CH.p(isc) if in_bn else None, CH.p(ish) if in_bn else None,
                                                        io16, st()))
            tdx.check(tdx.lib.tdx_conv3x3_wgrad_reduce(slabs.data_ptr(), dw.data_ptr(), splits, cout, cin, st()))
            torch.cuda.synchronize()
            kernel = BC.wgrad_kernel(shape, in_bn, io16, knobs).split("<")[0]
            ok, fig = BC.held(dw, regime, r["ref"], None, r["mag"], r["K"])
            note(kernel, regime, fig)
            print(f"{_wgrad_id(run)} in_bn={in_bn} {kernel}: {fig:.3g}")
            if not ok:
                fails.append(f"in_bn={in_bn} {kernel}: {fig:.3g}")
            if bool(torch.isnan(slabs).any()):
                fails.append(f"in_bn={in_bn}: a slab element was not written")
        if not guards.intact():
            fails.append("guard region written")
    assert not fails, fails


@pytest.mark.parametrize("cout,cin", BC.PACK_SHAPES)
def test_pack_is_the_permuted_rounded_weight_bit_for_bit(tdx, cout, cin):
    g = torch.Generator().manual_seed(cout + cin)
    d = {"w": torch.randn(cout, cin, 3, 3, generator=g)}
    d["w"][0, 0, 0, 0] = 1.0 + 2.0 ** -8          # a tie: nearest even is 1.0
    d["w"][0, 0, 0, 1] = 1.0 + 3 * 2.0 ** -8      # a tie: nearest even is 1 + 2^-6
    wf, wg = packs(tdx, d, cout, cin)
    rf, rg = BC.pack_refs(d["w"])
    assert torch.equal(wf.cpu().view(cout, 9, cin), rf) and torch.equal(wg.cpu().view(cin, 9, cout), rg)
    assert float(rf[0, 0, 0]) == 1.0 and float(rf[0, 1, 0]) == 1.0 + 2.0 ** -6
