"""CPU checks of the per-layer references and gate of tests/test_layer_taps_gpu.py (tests/_layer_reference.py):
the fp64 helpers reproduce the fp32 oracle, the 16-bit emulation's error is on the scale of the 16-bit type, the gate
constants cover the spread between two correct emulations, and the gate sees injected defects at the layer they are in.

Inputs: the full-size stacks (d = 1024 / 512) with the full-strength seed-0 weights over 3 + 3 layers, Gaussian encoder input
rows (the scale of post_extract_proj's output) and a 16-bit Gaussian conformer input; the mutations sit at layer K."""
import pytest
import torch

from tests import _layer_reference as lr

LAYERS, K = 3, 1
N = 100                                           # encoder rows; the conformer gets 2N, as after the x2 repeat
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
UNIT = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}    # unit roundoff

# Which injected defects the gate must see (and at which dtypes).  The others are smaller than the 16-bit noise of the layer
# they sit in, so a gate of the form e <= C * eps cannot see them (errors add in quadrature: a defect of size delta lifts e to
# sqrt(eps^2 + delta^2), past 2 x eps only once delta > sqrt(3) x eps); the test prints their measured defect/eps and does not
# assert that they stay unseen (a tighter gate or a closer emulation may see them):
# * ln_eps: eps 1e-5 vs 1e-12 rescales a row of variance ~1 by 5e-6 - 60x below fp16's layer error, 500x below bf16's (the
#   "defect/eps" of ~0.5 the table prints is the 16-bit re-rounding that this tiny rescale sets off, not the defect itself);
# * gelu_tanh: the tanh form departs from erf-GELU by <= 3e-4 absolute, below the 16-bit rounding of the hidden activations
#   themselves (|GELU| ~ 1: fp16 step 4.9e-4, bf16 3.9e-3);
# * pad_key in bf16: one zero-score key adds exp(-max score) to a softmax row sum - a few 1e-3 relative at these scores, the
#   size of bf16's own rounding of P (fp16, 8x finer, sees it).
# A padded key of a real clip carries the padded row's own K, not zeros; the GPU points B and C check that case at full depth.
MUST_TRIP = {("ln_eps", "conf"): (), ("drop_bias", "enc"): ("fp16", "bf16"), ("rel_shift", "conf"): ("fp16", "bf16"),
             ("pad_key", "enc"): ("fp16",), ("pad_key", "conf"): ("fp16",), ("gelu_tanh", "enc"): ()}


@pytest.fixture(scope="module")
def stacks():
    from lip2speech_unit_amd import ops, weights
    from lip2speech_unit_amd.model_avhubert import MultiTargetAVHubertEncoderModel
    model = MultiTargetAVHubertEncoderModel.build_model(dtype=ops.F16)
    keep = [lr.ENC + ".pos_conv", lr.ENC + ".layer_norm", lr.CONF + ".embed", lr.CONF + ".after_norm"]
    keep += [f"{lr.ENC}.layers.{i}." for i in range(LAYERS)] + [f"{lr.CONF}.encoders.{i}." for i in range(LAYERS)]
    spec = [(k, s) for k, s in weights.spec_of(model) if k.startswith(tuple(keep))]
    del model
    sd = weights.synth_state_dict(spec, seed=0)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, 1024, generator=g)
    xin = torch.randn(2 * N, 512, generator=g)
    ref = {"enc": lr.encoder_fp64(lr.sd64(sd, lr.ENC), x, LAYERS),
           "conf": {name: lr.conformer_fp64(lr.sd64(sd, lr.CONF), xin.to(t).float(), LAYERS) for name, t in T16.items()}}
    return sd, x, xin, ref


def _run(stacks, stack, name, splits=1, mut=None):
    sd, x, xin, ref = stacks
    t16 = T16[name]
    if stack == "enc":
        return lr.encoder_emulated(sd, x, t16, LAYERS, splits=splits, mut=mut), ref["enc"]
    return lr.conformer_emulated(sd, xin.to(t16).float(), t16, LAYERS, splits=splits, mut=mut), ref["conf"][name]


def test_fp64_reference_reproduces_the_fp32_oracle(stacks):
    from oracle import avhubert as oa
    from oracle import conformer as oc
    sd, x, xin, ref = stacks
    taps = {}
    with torch.no_grad():
        oa.transformer_encoder(sd, lr.ENC, x[None], None, 2, taps=taps)
        oc.espnet_encoder_after_frontend(sd, lr.CONF, xin.half().float()[None], torch.ones(1, 1, 2 * N, dtype=torch.bool), 2,
                                         taps=taps)
    for i in range(2):
        for got, want in ((taps[f"layer{i}"][0], ref["enc"][i]), (taps[f"block{i}"][0], ref["conf"]["fp16"][i])):
            e = float((got.double() - want).norm() / want.norm())
            assert 0 < e < 5e-6, (i, e)              # fp32 rounding (measured 3e-7 ... 5e-7)


@pytest.mark.parametrize("name", ["fp16", "bf16"])
@pytest.mark.parametrize("stack", ["enc", "conf"])
def test_emulation_error_is_16bit_sized(stacks, stack, name):
    emu, ref = _run(stacks, stack, name)
    e, w, _ = lr.errors(emu[0], ref[0])
    print(f"\n{stack} {name}: layer-0 emulation error {e:.3e} = {e / UNIT[name]:.2f} x unit roundoff, worst row {w:.3e}")
    assert 0.1 * UNIT[name] < e < 2 * UNIT[name], e
    assert e <= w < 4 * UNIT[name], w


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_gate_constants_cover_the_emulation_spread(stacks, name):
    """The committed constants were derived at full depth and the point shapes (tools/layer_gate_rho.py, through the same
    lr.emulation_spread); on this small stack the two emulations must still sit well inside them."""
    sd, x, xin, _ = stacks
    for stack, (rho_f, rho_r, _, _) in lr.emulation_spread(sd, x, xin.to(T16[name]).float(), T16[name], LAYERS, LAYERS).items():
        print(f"\n{stack} {name}: rho Frobenius {rho_f:.3f}, worst row {rho_r:.3f}")
        assert max(2.0, 1.5 * rho_f) <= lr.C_FROB and max(2.0, 1.5 * rho_r) <= lr.C_ROW, (stack, rho_f, rho_r)
    for stack in ("enc", "conf"):
        a, ref = _run(stacks, stack, name)
        b, _ = _run(stacks, stack, name, splits=8)
        ea, eb = lr.layer_errors(a, ref), lr.layer_errors(b, ref)
        assert lr.gate(eb, ea)[0] is None and lr.gate(ea, eb)[0] is None


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("row", [0, 57, N - 1])
def test_non_finite_tap_trips_the_gate_at_its_layer(stacks, bad, row):
    """One non-finite value in one valid row of one layer's tap fails that layer (NaN compares false both ways: the gate must
    not read it as a pass), and names the row; a non-finite emulation error fails too instead of skipping the layer."""
    base, ref = _run(stacks, "enc", "fp16")
    eb = lr.layer_errors(base, ref)
    tap = [t.clone() for t in base]
    tap[K][row, 3] = bad
    layer, msg, _ = lr.gate(lr.layer_errors(tap, ref), eb)
    assert layer == K and f"t={row}" in msg, (layer, msg)
    # NaN propagated down the stream: still the first such layer
    for t in tap[K + 1:]:
        t[:, :] = bad
    assert lr.gate(lr.layer_errors(tap, ref), eb)[0] == K
    # a broken emulation is a failure, not a reported layer
    assert lr.gate(eb, lr.layer_errors(tap, ref))[0] == K


def test_mutations_trip_the_gate_at_their_layer(stacks):
    rows, bad = [], []
    for (kind, stack), must in MUST_TRIP.items():
        for name in T16:
            base, ref = _run(stacks, stack, name)
            mut, _ = _run(stacks, stack, name, mut=(kind, stack, K))
            eb, em = lr.layer_errors(base, ref), lr.layer_errors(mut, ref)
            layer, msg, rep = lr.gate(em, eb)
            delta = float((mut[K] - base[K]).norm() / ref[K].norm()) / eb[K][0]
            rows.append(f"  {kind:10s} {stack:5s} {name}  e/eps {em[K][0] / eb[K][0]:7.2f}  w/omega {em[K][1] / eb[K][1]:7.2f}  "
                        f"defect/eps {delta:7.2f}  tripped at {layer}" + ("" if name in must else "  (below the noise: reported)"))
            assert not rep
            if name in must and layer != K:
                bad.append(f"{kind} {stack} {name}: gate tripped at {layer}, not at layer {K}")
            elif layer is not None and layer != K:        # the layers before K are the unmutated stack
                bad.append(f"{kind} {stack} {name}: gate tripped at {layer}, before the mutated layer {K}")
    for stack in ("enc", "conf"):                    # reported, not asserted
        for name in T16:
            base, ref = _run(stacks, stack, name)
            mut, _ = _run(stacks, stack, name, mut=("res16", stack, K))
            eb, em = lr.layer_errors(base, ref), lr.layer_errors(mut, ref)
            rows.append(f"  {'res16':10s} {stack:5s} {name}  e/eps {em[K][0] / eb[K][0]:7.2f}  w/omega {em[K][1] / eb[K][1]:7.2f}  "
                        f"tripped at {lr.gate(em, eb)[0]}  (report only)")
    print(f"\nmutation table (layer {K} of {LAYERS}, gate C_FROB {lr.C_FROB:g} / C_ROW {lr.C_ROW:g}):\n" + "\n".join(rows))
    assert not bad, "\n".join(bad)
