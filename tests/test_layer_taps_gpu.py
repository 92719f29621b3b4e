"""Per-layer parity at full depth and full branch strength: the fp32 residual stream after each of the 24 AV-HuBERT layers and
the 12 conformer blocks, tapped from the HIP run, against an fp64 reference of the same stack (tests/_layer_reference.py) -
at each operating point that selects a different kernel:

  A  B = 32, T = 100, lens {1: 73, 3: 40}; clips 0-3: one-launch phase GEMMs, tiled plain attention, resident rel-pos at T = 200
  B  B = 2, lens [100, 37]: M <= 512, split-K + splitk_reduce_layernorm in every layer, with a mask
  C  B = 2, lens [600, 25] (24 s and 1 s): encoder attention on 128-row query blocks (T = 600), conformer rel-pos T = 1200
     (2 399 positions) on the tiled kernel, GLU-dwconv T = 1200, 575 padded keys in clip 1

Each stack is measured on its own: the references start from the input the HIP stack itself was given (captured by
`layer_taps`) and run each checked clip ALONE over its valid rows.  Per layer i and clip, against the fp64 stream:
e_i / w_i = relative Frobenius / worst per-row relative error of the GPU tap, eps_i / omega_i = the same of the 16-bit
emulation.  Gate: e_i <= C_FROB * eps_i and w_i <= C_ROW * omega_i (constants and their CPU derivation in
tests/_layer_reference.py); a layer whose emulation error exceeds MEANINGLESS is reported, not gated."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import conformer as conf_mod  # noqa: E402
from lip2speech_unit_amd import hubert, ops, weights  # noqa: E402
from lip2speech_unit_amd.model_avhubert import MultiTargetAVHubertEncoderModel  # noqa: E402
from lip2speech_unit_amd.pipeline import LipToSpeechPipeline  # noqa: E402
from tests import _layer_reference as lr  # noqa: E402
from tests.test_models_gpu import _frames  # noqa: E402

ENC_LAYERS, CONF_LAYERS = 24, 12
POINTS = {
    "A": dict(B=32, T=100, lens={1: 73, 3: 40}, clips=(0, 1, 2, 3)),
    "B": dict(B=2, T=100, lens={1: 37}, clips=(0, 1)),
    "C": dict(B=2, T=600, lens={1: 25}, clips=(0, 1)),
}
NAME = {ops.F16: "fp16", ops.BF16: "bf16"}


@contextlib.contextmanager
def layer_taps():
    """Eager-run taps of the two stacks without touching the product: the input of TransformerEncoder.forward_rows and of
    conformer Encoder.forward_rows, and a clone of the fp32 residual stream x after every ops.residual_linear call with
    key "w2" (the end of an encoder layer) or "ff" (the end of a conformer block: norm_final is applied to x in place there)."""
    got = {"enc_in": None, "conf_in": None, "enc": [], "conf": []}
    rl, enc_fr, conf_fr = ops.residual_linear, hubert.TransformerEncoder.forward_rows, conf_mod.Encoder.forward_rows

    def residual_linear(A, W, bias, x, **kw):
        rl(A, W, bias, x, **kw)
        if kw.get("key") == "w2":
            got["enc"].append(x.clone())
        elif kw.get("key") == "ff":
            got["conf"].append(x.clone())

    def encoder_rows(self, x32, x16, lens, B, T):
        got["enc_in"] = (x32.clone(), x16.clone(), lens.clone(), B, T)
        return enc_fr(self, x32, x16, lens, B, T)

    def conformer_rows(self, xin, lens, B, T, len_mul, dtype):
        got["conf_in"] = (xin.clone(), lens.clone(), B, T, len_mul)
        return conf_fr(self, xin, lens, B, T, len_mul, dtype)

    ops.residual_linear = residual_linear
    hubert.TransformerEncoder.forward_rows = encoder_rows
    conf_mod.Encoder.forward_rows = conformer_rows
    try:
        yield got
    finally:
        ops.residual_linear = rl
        hubert.TransformerEncoder.forward_rows = enc_fr
        conf_mod.Encoder.forward_rows = conf_fr


@pytest.fixture(scope="module")
def taps_setup():
    """Full-strength weights (seed 0, as full_setup of tests/test_fulldepth_gpu.py), their fp64 stack copies, and one model
    per dtype built on first use."""
    model = MultiTargetAVHubertEncoderModel.build_model(dtype=ops.F16)
    sd = weights.synth_state_dict(weights.spec_of(model), seed=0)
    del model
    return {"sd": sd, "enc64": lr.sd64(sd, lr.ENC), "conf64": lr.sd64(sd, lr.CONF), "models": {}}


def _model(setup, dt):
    if dt not in setup["models"]:
        m = MultiTargetAVHubertEncoderModel.build_model(dtype=dt)
        m.load_state_dict(setup["sd"])
        setup["models"][dt] = m.cuda().eval()
    return setup["models"][dt]


@pytest.mark.parametrize("dt", [ops.F16, ops.BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("point", sorted(POINTS))
def test_layer_taps_vs_fp64(taps_setup, point, dt):
    P = POINTS[point]
    B, T, lens = P["B"], P["T"], P["lens"]
    sd, t16, name = taps_setup["sd"], ops.torch_dtype(dt), NAME[dt]
    model = _model(taps_setup, dt)
    video = _frames(B, T, 2024)
    pad = torch.zeros(B, T, dtype=torch.bool)
    for b, n in lens.items():
        pad[b, n:] = True
        video[b, :, n:] = 0
    g = torch.Generator().manual_seed(7)
    spk = torch.rand(B, 256, generator=g).relu()
    spk = spk / spk.norm(dim=-1, keepdim=True)
    with layer_taps() as got, torch.no_grad():
        LipToSpeechPipeline(model, None).stage1_device(video.cuda(), pad.cuda(), spk.cuda())
        torch.cuda.synchronize()
    # a refactor that bypasses the hooks must fail here, not leave the test checking nothing
    assert len(got["enc"]) == ENC_LAYERS and len(got["conf"]) == CONF_LAYERS, (len(got["enc"]), len(got["conf"]))
    x32, x16, _, Be, Te = got["enc_in"]
    xin, _, Bc, T2, len_mul = got["conf_in"]
    assert (Be, Te, Bc, T2, len_mul) == (B, T, B, 2 * T, 2)
    x32, x16, xin = x32.float().cpu(), x16.float().cpu(), xin.float().cpu()
    enc = [t.cpu().view(B, T, -1) for t in got["enc"]]
    conf = [t.cpu().view(B, T2, -1) for t in got["conf"]]
    failures, reported, worst = [], {"enc": 0, "conf": 0}, {}
    for b in P["clips"]:
        n = lens.get(b, T)
        for stack, rows, ref_fn, emu_fn, tap in (
                ("enc", n, lambda: lr.encoder_fp64(taps_setup["enc64"], x32[b * T:b * T + n], ENC_LAYERS),
                 lambda: lr.encoder_emulated(sd, x32[b * T:b * T + n], t16, ENC_LAYERS, x16=x16[b * T:b * T + n]), enc),
                ("conf", 2 * n, lambda: lr.conformer_fp64(taps_setup["conf64"], xin[b * T2:b * T2 + 2 * n], CONF_LAYERS),
                 lambda: lr.conformer_emulated(sd, xin[b * T2:b * T2 + 2 * n], t16, CONF_LAYERS), conf)):
            ref = ref_fn()
            emu = lr.layer_errors(emu_fn(), ref)
            gpu = lr.layer_errors([t[b, :rows] for t in tap], ref)
            print(f"\n[layer taps {point} {name}] {stack} clip {b} ({rows} rows)\n" + lr.table(gpu, emu))
            layer, msg, rep = lr.gate(gpu, emu)
            reported[stack] += len(rep)
            if layer is not None:
                failures.append(f"point {point} {name} {stack} clip {b}: {msg}")
            for i, ((e, w, t), (eps, om, _)) in enumerate(zip(gpu, emu)):
                for k, v in (("e/eps", e / eps), ("w/omega", w / om)):
                    if v > worst.get((stack, k), (0.0,))[0]:
                        worst[(stack, k)] = (v, i, b, t)
    print(f"\n[layer taps {point} {name}] worst ratios: " + "; ".join(
        f"{s} {k} {v[0]:.2f} (layer {v[1]}, clip {v[2]}, row {v[3]})" for (s, k), v in sorted(worst.items()))
          + f"; layers reported instead of gated: enc {reported['enc']}, conf {reported['conf']}")
    assert not failures, "\n".join(failures)
