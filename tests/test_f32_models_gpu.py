"""Stage 1 in fp32 (ops.F32, the reference's default precision) at module and model level.

FIXTURES.  The reference-pinned fixtures, checked at 4 x max|golden - fp64 evaluation of the same module| (floor 2^-20 *
max|golden|; tests/_f32_fixtures.py) - the reference's own fp32 rounding as frozen in the file, nothing from the GPU.  Measured
on the CPU (python -c "from tests import _f32_fixtures as f; ..." over all_fixture_references):

    fixture                      max|golden - fp64|   max|golden|   tolerance    of scale    16-bit test's tolerance (fp16)
    frontend.npz out                  5.91e-06           18.37      2.36e-05     1.3e-06     1e-2   (7 800 x looser)
    frontend.npz stem_t2              3.63e-03           10.70      1.45e-02     1.4e-03     4e-3   (see below)
    conformer.npz out[0]              2.77e-06            3.77      1.11e-05     2.9e-06     1.5e-2 (5 100 x)
    conformer.npz out_clip1_alone     2.85e-06            3.80      1.14e-05     3.0e-06     1.5e-2 (5 000 x)
    hubert_standin.npz out            3.50e-06            5.20      1.40e-05     2.7e-06     6e-3   (2 200 x)

stem_t2 is the one tolerance above 1/100 of the 16-bit one, and the cause is the fixture, not the reference's arithmetic: the
tap was STORED as float16 (dtype of the array in the .npz), so its distance from fp64 is half a float16 ulp at |x| ~ 10
(2^-8 = 3.9e-03), and no check against this file can be tighter than that.  The stem is held to the fp32 scale by
tests/test_f32_kernels_gpu.py::test_stem_pool_avgpool (fp64 reference, 4 x torch's float32 error) and, through the whole
frontend, by `out` above.

FULL DEPTH.  Setup of tests/test_fulldepth_gpu.py (seed 0, B = 32, T = 100, lens {1: 73, 3: 40}, clips 0-3 against the oracle
run on each clip alone): all 626 unit ids equal, no frame skipped, and max |logit err| < 3.7e-4 = half the smallest oracle
top-2 margin (7.41e-4; the next is 2.21e-2).

PER-LAYER TAPS at points A, B, C of tests/test_layer_taps_gpu.py (`layer_taps` reused): truth encoder_fp64 / conformer_fp64,
yardstick the float32 evaluation (`*_emulated` with t16 = float32), gate constants tests/_f32_reference.py.

GRAPH REPLAY bit for bit, and the CLI with dtype=f32."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import ops, weights  # noqa: E402
from lip2speech_unit_amd.conformer import Conformer, ConformerConfig  # noqa: E402
from lip2speech_unit_amd.hubert import AVHubertConfig, TransformerEncoder  # noqa: E402
from lip2speech_unit_amd.model_avhubert import MultiTargetAVHubertEncoderModel  # noqa: E402
from lip2speech_unit_amd.pipeline import GraphCache, LipToSpeechPipeline  # noqa: E402
from tests import _f32_fixtures as fx  # noqa: E402
from tests import _f32_reference as fr  # noqa: E402
from tests import _layer_reference as lr  # noqa: E402
from tests.test_models_gpu import _frames, _run_conformer_blocks  # noqa: E402

DT = ops.F32


def _check_fixture(name, got, gold, ref64, tol16):
    tol, dev, scale = fx.tolerance(gold, ref64)
    err = (got.double() - gold.double()).abs().max().item()
    err64 = (got.double() - ref64).abs().max().item()
    print(f"\n[f32 fixtures] {name}: max |gpu - golden| {err:.3e} (tolerance {tol:.3e} = 4 x {dev:.3e}; {tol / scale:.2e} of max|golden| "
          f"{scale:.3e}; the fp16 test allows {tol16:g} of scale); max |gpu - fp64| {err64:.3e}")
    assert torch.isfinite(got).all()
    assert err <= tol, f"{name}: {err:.3e} > {tol:.3e}"
    return tol / scale


def test_frontend_fixture(golden_dir):
    from lip2speech_unit_amd.resnet import ResEncoder
    f = fx.frontend(golden_dir)
    enc = ResEncoder("prelu", None, dtype=DT)
    enc.load_state_dict(f["sd"])
    enc = enc.cuda().eval()
    with torch.no_grad():
        got = enc(f["x"].cuda()).cpu()
    rel = _check_fixture("frontend.npz out", got, *f["out"], tol16=1e-2)
    assert rel < 1e-2 / 100
    # the stem tap of frame 2 (stored as float16 in the fixture: see the header)
    P = enc._packed
    B, T = f["x"].shape[0], f["x"].shape[2]
    y = torch.empty(B * T, 44, 44, 64, device="cuda")
    ops.stem_conv3d(f["x"][:, 0].contiguous().cuda(), P["stem_w"], P["stem_b"], P["stem_s"], y, B, T, DT)
    _check_fixture("frontend.npz stem_t2", y[2].permute(2, 0, 1).cpu(), *f["stem_t2"], tol16=4e-3)


def test_conformer_fixture(golden_dir):
    c = fx.conformer(golden_dir)
    con = Conformer(ConformerConfig(), dtype=DT)
    con.encoder.load_state_dict(c["esd"])
    con = con.cuda().eval()
    con.pack("cuda")
    y = _run_conformer_blocks(con, c["x"], c["lens"].int().cuda(), DT)
    n = c["out_clip1_alone"][0].shape[0]
    rel0 = _check_fixture("conformer.npz out[0]", y[0], *c["out0"], tol16=1.5e-2)
    rel1 = _check_fixture("conformer.npz out_clip1_alone", y[1, :n], *c["out_clip1_alone"], tol16=1.5e-2)
    assert max(rel0, rel1) < 1.5e-2 / 100


def test_hubert_standin_fixture(golden_dir):
    h = fx.hubert_standin(golden_dir)
    enc = TransformerEncoder(AVHubertConfig(encoder_layers=h["layers"]), dtype=DT)
    enc.load_state_dict({k[4:]: v for k, v in h["sd"].items()})
    x, pad = h["x"], h["pad"]
    B, T, C = x.shape
    x32 = x.masked_fill(pad[:, :, None], 0.0).reshape(B * T, C).cuda()
    out = enc.forward_rows(x32, x32.clone(), h["lens"].int().cuda(), B, T).cpu().view(B, T, C)
    valid = ~pad
    rel = _check_fixture("hubert_standin.npz out", out[valid], h["out"][0][valid], h["out"][1][valid], tol16=6e-3)
    assert rel < 6e-3 / 100


# ---- full depth ------------------------------------------------------------------------------------------------------------

B, T = 32, 100
ORACLE_CLIPS = (0, 1, 2, 3)
LENS = {1: 73, 3: 40}
MAX_LOGIT_ERR = 3.7e-4      # half the smallest oracle top-2 margin of the 626 frames (7.41e-4), computed on the CPU


@pytest.fixture(scope="module")
def full():
    model = MultiTargetAVHubertEncoderModel.build_model(dtype=DT)
    sd = weights.synth_state_dict(weights.spec_of(model), seed=0)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    video = _frames(B, T, 2024)
    pad = torch.zeros(B, T, dtype=torch.bool)
    for b, n in LENS.items():
        pad[b, n:] = True
        video[b, :, n:] = 0
    g = torch.Generator().manual_seed(7)
    spk = torch.rand(B, 256, generator=g).relu()
    spk = spk / spk.norm(dim=-1, keepdim=True)
    return {"sd": sd, "model": model, "video": video, "pad": pad, "spk": spk}


def test_full_depth_all_unit_ids_exact(full):
    from oracle import stage1 as os1
    video, pad, spk = full["video"], full["pad"], full["spk"]
    out = LipToSpeechPipeline(full["model"], None).stage1_device(video.cuda(), pad.cuda(), spk.cuda())
    torch.cuda.synchronize()
    n_tot = n_diff = 0
    logit_err = mel_err = 0.0
    min_margin = float("inf")
    for b in ORACLE_CLIPS:
        n = LENS.get(b, T)
        L = 2 * n
        with torch.no_grad():
            ref = os1.generate(full["sd"], video[b:b + 1, :, :n], torch.zeros(1, n, dtype=torch.bool), spk[b:b + 1])
        lg = ref["logits"][:L, 0]
        top2 = lg[:, 4:].topk(2, -1).values
        min_margin = min(min_margin, float((top2[:, 0] - top2[:, 1]).min()))
        toks = out["tokens"][b].cpu().long()
        n_tot += L
        n_diff += int((toks[:L] != ref["tokens"][0][:L]).sum())
        assert toks[L].item() == 2 and (toks[L + 1:] == 1).all()
        logit_err = max(logit_err, float((out["logits"][b, :L].cpu() - lg).abs().max()))
        mel_err = max(mel_err, float((out["mel"][b, : 2 * L].cpu() - ref["mels"][0]).abs().max()))
    print(f"\n[full-depth f32] {n_tot - n_diff}/{n_tot} unit ids equal the oracle's (no frame skipped); max |logit err| {logit_err:.3e} "
          f"(gate {MAX_LOGIT_ERR:g}; smallest oracle top-2 margin {min_margin:.3e}); mel max abs err {mel_err:.3e}")
    assert n_tot == 626
    assert n_diff == 0, f"{n_diff} of {n_tot} unit ids differ"
    assert logit_err < MAX_LOGIT_ERR, logit_err


# ---- per-layer taps ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("point", ["A", "B", "C"])
def test_layer_taps_f32_vs_fp64(full, point):
    from tests.test_layer_taps_gpu import CONF_LAYERS, ENC_LAYERS, POINTS, layer_taps
    P = POINTS[point]
    Bp, Tp, lens = P["B"], P["T"], P["lens"]
    sd, model = full["sd"], full["model"]
    enc64, conf64 = lr.sd64(sd, lr.ENC), lr.sd64(sd, lr.CONF)
    video = _frames(Bp, Tp, 2024)
    pad = torch.zeros(Bp, Tp, dtype=torch.bool)
    for b, n in lens.items():
        pad[b, n:] = True
        video[b, :, n:] = 0
    g = torch.Generator().manual_seed(7)
    spk = torch.rand(Bp, 256, generator=g).relu()
    spk = spk / spk.norm(dim=-1, keepdim=True)
    with layer_taps() as got, torch.no_grad():
        LipToSpeechPipeline(model, None).stage1_device(video.cuda(), pad.cuda(), spk.cuda())
        torch.cuda.synchronize()
    assert len(got["enc"]) == ENC_LAYERS and len(got["conf"]) == CONF_LAYERS, (len(got["enc"]), len(got["conf"]))
    x32, x16, _, Be, Te = got["enc_in"]
    xin, _, Bc, T2, len_mul = got["conf_in"]
    assert (Be, Te, Bc, T2, len_mul) == (Bp, Tp, Bp, 2 * Tp, 2)
    assert x16.dtype == torch.float32 and xin.dtype == torch.float32 and torch.equal(x16, x32)
    x32, xin = x32.cpu(), xin.cpu()
    enc = [t.cpu().view(Bp, Tp, -1) for t in got["enc"]]
    conf = [t.cpu().view(Bp, T2, -1) for t in got["conf"]]
    failures, worst = [], {}
    for b in P["clips"]:
        n = lens.get(b, Tp)
        for stack, rows, ref_fn, emu_fn, tap in (
                ("enc", n, lambda: lr.encoder_fp64(enc64, x32[b * Tp:b * Tp + n], ENC_LAYERS),
                 lambda: lr.encoder_emulated(sd, x32[b * Tp:b * Tp + n], torch.float32, ENC_LAYERS), enc),
                ("conf", 2 * n, lambda: lr.conformer_fp64(conf64, xin[b * T2:b * T2 + 2 * n], CONF_LAYERS),
                 lambda: lr.conformer_emulated(sd, xin[b * T2:b * T2 + 2 * n], torch.float32, CONF_LAYERS), conf)):
            with torch.no_grad():
                ref = ref_fn()
                emu = lr.layer_errors(emu_fn(), ref)
            gpu = lr.layer_errors([t[b, :rows] for t in tap], ref)
            print(f"\n[layer taps {point} f32] {stack} clip {b} ({rows} rows)\n" + lr.table(gpu, emu))
            layer, msg, rep = lr.gate(gpu, emu, c=fr.C_FROB_F32, c_row=fr.C_ROW_F32)
            assert not rep, rep          # a float32 evaluation's error is never "meaningless"
            if layer is not None:
                failures.append(f"point {point} f32 {stack} clip {b}: {msg}")
            for i, ((e, w, t), (eps, om, _)) in enumerate(zip(gpu, emu)):
                for k, v in (("e/eps", e / eps), ("w/omega", w / om)):
                    if v > worst.get((stack, k), (0.0,))[0]:
                        worst[(stack, k)] = (v, i, b, t)
    print(f"\n[layer taps {point} f32] gates {fr.C_FROB_F32:.2f} / {fr.C_ROW_F32:.2f}; worst ratios: " + "; ".join(
        f"{s} {k} {v[0]:.2f} (layer {v[1]}, clip {v[2]}, row {v[3]})" for (s, k), v in sorted(worst.items())))
    assert not failures, "\n".join(failures)


# ---- graph replay, text head, CLI ------------------------------------------------------------------------------------------------


def _small(text=False, seed=3):
    ccfg = ConformerConfig(conformer_layers=2)
    ccfg.text_supervision = text
    if text:
        ccfg.text_classes = 39
    m = MultiTargetAVHubertEncoderModel.build_model(dtype=DT, w2v_cfg=AVHubertConfig(encoder_layers=2), conformer_cfg=ccfg)
    m.load_state_dict(weights.synth_state_dict(weights.spec_of(m), seed=seed))
    return m.cuda().eval()


@pytest.mark.parametrize("text", [False, True], ids=["units", "text_head"])
def test_graph_replay_equals_eager_bit_for_bit(text):
    m = _small(text)
    pipe = LipToSpeechPipeline(m, None)
    Bs, Ts = 3, 13
    keys = ("tokens", "lprobs", "score", "mel", "logits") + (("text", "text_logits") if text else ())

    def fn(video, pad, spk):
        o = pipe.stage1_device(video, pad, spk)
        return tuple(o[k] for k in keys)
    cache = GraphCache(fn)
    for seed, lens in ((1, [13, 9, 4]), (2, [5, 13, 13])):
        video = _frames(Bs, Ts, seed)
        pad = torch.zeros(Bs, Ts, dtype=torch.bool)
        for b, n in enumerate(lens):
            pad[b, n:] = True
            video[b, :, n:] = 0
        spk = torch.rand(Bs, 256, generator=torch.Generator().manual_seed(seed))
        eager = [t.clone() for t in fn(video.cuda(), pad.cuda(), spk.cuda())]
        replay = [t.clone() for t in cache(video.cuda(), pad.cuda(), spk.cuda())]
        torch.cuda.synchronize()
        for k, a, b_ in zip(keys, eager, replay):
            assert torch.equal(a, b_), f"{k}: graph replay differs from the eager run"
        assert torch.isfinite(eager[3]).all()
    assert cache.captures == 1
    if text:
        # the text head is one more fp32 tap-GEMM: its logits equal an fp64 evaluation of the Linear to fp32 rounding
        o = pipe.stage1_device(video.cuda(), pad.cuda(), spk.cuda())
        assert o["text"].dtype == torch.int32 and o["text_logits"].shape[:2] == (Bs, 2 * Ts)


def test_cli_dtype_f32(tmp_path):
    from lip2speech_unit_amd import inference as s1
    from tests._synth_dataset import make
    lab = make(str(tmp_path / "ds"), frames=(12, 9, 5))
    out = {}
    for dt in ("f32", "f16"):
        out[dt] = str(tmp_path / ("out_" + dt))
        res = s1.main([f"common_eval.results_path={out[dt]}", f"override.data={lab}", f"override.label_dir={lab}",
                       "synthetic_weights=true", "dataset.batch_size=2", "model.encoder_layers=2", "model.conformer_layers=2",
                       f"dtype={dt}"])
        assert len(res["utt_id"]) == 3
    for utt, Tn in zip(("test/spk0/00000", "test/spk1/00001", "test/spk0/00002"), (12, 9, 5)):
        units = open(os.path.join(out["f32"], "pred_unit", utt + ".txt")).read().split()
        assert len(units) == 2 * Tn and all(0 <= int(u) < 200 for u in units)
        mel = np.load(os.path.join(out["f32"], "pred_mel", utt + ".npy"))
        assert mel.shape == (4 * Tn, 80) and mel.dtype == np.float32 and np.isfinite(mel).all()
        mel16 = np.load(os.path.join(out["f16"], "pred_mel", utt + ".npy"))
        d = np.abs(mel - mel16).max()
        assert 0 < d < 3e-2, d            # the two precisions are different computations of the same model
