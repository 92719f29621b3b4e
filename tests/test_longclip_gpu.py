"""Mixed-length batch with a 10-s clip (BASELINE configs[4] shape family): every stage incl. the vocoder against the
clip-alone oracle.  Exercises the big-tile / patch / fused-ResBlock kernels with row masks at realistic sizes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import ops, weights  # noqa: E402
from lip2speech_unit_amd.conformer import ConformerConfig  # noqa: E402
from lip2speech_unit_amd.hubert import AVHubertConfig  # noqa: E402
from lip2speech_unit_amd.model_avhubert import MultiTargetAVHubertEncoderModel  # noqa: E402
from lip2speech_unit_amd.pipeline import LipToSpeechPipeline  # noqa: E402
from lip2speech_unit_amd.vocoder import AttrDict, MelCodeGenerator  # noqa: E402
from oracle import stage1 as os1  # noqa: E402
from oracle import vocoder as ov  # noqa: E402
from tests.test_models_gpu import VOC_H, _frames  # noqa: E402


def test_mixed_length_batch_with_10s_clip():
    dt = ops.F16
    model = MultiTargetAVHubertEncoderModel.build_model(dtype=dt, w2v_cfg=AVHubertConfig(encoder_layers=2),
                                                        conformer_cfg=ConformerConfig(conformer_layers=2))
    sd = weights.synth_state_dict(weights.spec_of(model), seed=41)
    model.load_state_dict(sd)
    voc = MelCodeGenerator(AttrDict(VOC_H), dtype=dt)
    vsd = weights.synth_state_dict(weights.spec_of(voc), seed=42)
    voc.load_state_dict(vsd)
    voc.remove_weight_norm()
    model.cuda().eval()
    voc.cuda().eval()
    lens = [250, 111, 25]                      # 10 s, 4.4 s, 1 s
    B, T = len(lens), max(lens)
    video = _frames(B, T, 123)
    pad = torch.zeros(B, T, dtype=torch.bool)
    for b, n in enumerate(lens):
        pad[b, n:] = True
        video[b, :, n:] = 0
    spk = torch.rand(B, 256, generator=torch.Generator().manual_seed(5))
    out = LipToSpeechPipeline(model, voc).forward_device(video.cuda(), pad.cuda(), spk.cuda())
    torch.cuda.synchronize()
    vsd_r = {k: v.detach().float().cpu() for k, v in voc.state_dict().items()}
    for b, n in enumerate(lens):
        with torch.no_grad():
            ref = os1.generate(sd, video[b:b + 1, :, :n], torch.zeros(1, n, dtype=torch.bool), spk[b:b + 1],
                               enc_layers=2, conf_layers=2)
        L = 2 * n
        lr = ref["logits"][:, 0, 4:]
        top2 = lr.topk(2, -1).values
        safe = (top2[:, 0] - top2[:, 1]) > 2e-2
        toks = out["tokens"][b].cpu().long()
        assert torch.equal(toks[:L][safe], ref["tokens"][0][:L][safe]), f"clip {b}"
        assert toks[L].item() == 2 and (toks[L + 1:] == 1).all()
        assert int((~safe).sum()) <= 0.1 * L
        mel = out["mel"][b, : 2 * L].cpu()
        assert (mel - ref["mels"][0]).abs().max().item() < 3e-2
        if bool(safe.all()):
            with torch.no_grad():
                code = (ref["tokens"][0][:-1] - 4).unsqueeze(0)
                wav = ov.mel_code_generator(vsd_r, VOC_H, code, ref["mels"][0].t().unsqueeze(0), spk[b:b + 1])[0, 0]
            got = out["wav"][b, : 320 * L].cpu()
            assert (got - wav).abs().max().item() < 2e-3, f"clip {b} wav"     # fp16: ~8x the measured 2.6e-4
        if 320 * L < out["wav"].shape[1]:
            assert out["wav"][b, 320 * L:].abs().max().item() == 0.0


# ---- a 24-s clip through the vocoder, teacher-forced (no stage 1): the service's longest clip next to a 1-s one ----------
VOC_LENS = (1200, 50)                          # unit frames (50 Hz): 24 s and 1 s -> 384 000 and 16 000 samples


@pytest.fixture(scope="module")
def voc24_setup():
    """Seed-1 vocoder weights (full_setup of tests/test_fulldepth_gpu.py), seeded unit ids, a smooth synthetic mel, speaker
    embeddings, and the oracle's waveform of each clip ALONE (computed once)."""
    voc = MelCodeGenerator(AttrDict(VOC_H), dtype=ops.F16)
    vsd = weights.synth_state_dict(weights.spec_of(voc), seed=1)
    voc.load_state_dict(vsd)
    voc.remove_weight_norm()
    vsd_r = {k: v.detach().float().cpu() for k, v in voc.state_dict().items()}
    B, L = len(VOC_LENS), max(VOC_LENS)
    g = torch.Generator().manual_seed(24)
    code = torch.randint(0, 200, (B, L), generator=g)
    t = torch.arange(2 * L, dtype=torch.float32)[None, None, :]
    f = torch.arange(80, dtype=torch.float32)[None, :, None]
    ph = torch.rand(B, 1, 1, generator=g) * 6.28
    mel = -6.0 + 2.5 * torch.sin(t / 37.0 + ph) * torch.cos(f / 13.0) + 1.5 * torch.cos(t / 11.0 + f / 7.0 + ph)
    spk = torch.rand(B, 256, generator=g).relu()
    spk = spk / spk.norm(dim=-1, keepdim=True)
    refs = []
    with torch.no_grad():
        for b, n in enumerate(VOC_LENS):
            refs.append(ov.mel_code_generator(vsd_r, VOC_H, code[b:b + 1, :n], mel[b:b + 1, :, :2 * n], spk[b:b + 1])[0, 0])
    return vsd, code, mel, spk, refs


@pytest.mark.parametrize("min_tiles", [0, 64])   # tests/test_models_gpu.py PAIR_MODES: tap-GEMM stages / fused conv pairs
@pytest.mark.parametrize("dt", [ops.F16, ops.BF16], ids=["fp16", "bf16"])
def test_vocoder_24s_clip_teacher_forced(voc24_setup, dt, min_tiles, monkeypatch):
    from lip2speech_unit_amd import vocoder as vmod
    from tests.test_fulldepth_gpu import WAV_TOL
    from tests.test_models_gpu import PAIR_MODES
    assert min_tiles in PAIR_MODES
    monkeypatch.setattr(vmod, "PAIR_MIN_TILES", min_tiles)
    vsd, code, mel, spk, refs = voc24_setup
    voc = MelCodeGenerator(AttrDict(VOC_H), dtype=dt)
    voc.load_state_dict(vsd)
    voc.remove_weight_norm()
    voc.cuda().eval()
    lens = torch.tensor(VOC_LENS, dtype=torch.int32)
    with torch.no_grad():
        wav, _ = voc.forward_rows(code.cuda(), mel.cuda(), spk.cuda(), lens.cuda())
    torch.cuda.synchronize()
    wav = wav.cpu()
    assert wav.shape == (2, 320 * max(VOC_LENS))
    for b, n in enumerate(VOC_LENS):
        S = 320 * n
        assert refs[b].shape == (S,)
        err = (wav[b, :S] - refs[b]).abs().max().item()
        print(f"vocoder 24-s batch, clip {b} ({S} samples, {'fp16' if dt == ops.F16 else 'bf16'}, min_tiles {min_tiles}): "
              f"max abs err {err:.3e}")
        assert err < WAV_TOL[dt], (b, err)
        if S < wav.shape[1]:
            assert wav[b, S:].abs().max().item() == 0.0
