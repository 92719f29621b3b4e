"""Reloading weights on the device: after a load_state_dict - through the root or through one child - every path runs the new
weights, bit for bit what a freshly built model with those weights gives (same weights, same kernels, same bits), and whatever
holds pointers into the old packed tensors (a GraphCache, the pipeline's primed shared state) notices."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from bench import synth_inputs  # noqa: E402
from lip2speech_unit_amd import ops, speaker_encoder  # noqa: E402
from lip2speech_unit_amd.packing import state_epoch  # noqa: E402
from lip2speech_unit_amd.pipeline import GraphCache, LipToSpeechPipeline  # noqa: E402
from lip2speech_unit_amd.vocoder import AttrDict, MelCodeGenerator  # noqa: E402
from tests import _tiny_models as tiny  # noqa: E402

B, T = 2, 8
KEYS = ("tokens", "mel", "logits")


def _model(seed):
    return tiny.loaded(lambda: tiny.avhubert(ffn=None), seed).cuda()


def _vocoder(seed):
    return tiny.loaded(lambda: MelCodeGenerator(AttrDict(tiny.VOC_H), dtype=ops.F16), seed).cuda()


@pytest.fixture(scope="module")
def inputs():
    video, spk, u8 = synth_inputs(B, T, seed=3, with_u8=True)
    return video.cuda(), spk.cuda(), u8.cuda()


def _stage1(model, video, spk):
    out = LipToSpeechPipeline(model, None).stage1_device(video, None, spk)
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in KEYS}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def test_reload_through_the_root(inputs):
    video, spk, _ = inputs
    m = _model(0)
    old = _stage1(m, video, spk)
    m.load_state_dict(tiny.synth(m, 1))
    new = _stage1(m, video, spk)
    assert _same(new, _stage1(_model(1), video, spk)) and not _same(new, old)


def test_reload_through_one_child(inputs):
    video, spk, _ = inputs
    m = _model(0)
    old = _stage1(m, video, spk)
    prefix = "encoder.w2v_model.encoder."
    part = {k: v for k, v in tiny.synth(m, 1).items() if k.startswith(prefix)}
    m.encoder.w2v_model.encoder.load_state_dict({k[len(prefix):]: v for k, v in part.items()})
    new = _stage1(m, video, spk)
    fresh = tiny.avhubert(ffn=None)
    fresh.load_state_dict(dict(tiny.synth(fresh, 0), **part))
    assert _same(new, _stage1(fresh.eval().cuda(), video, spk)) and not _same(new, old)


def test_vocoder_precise_path_after_a_reload():
    L = 8
    g = torch.Generator().manual_seed(4)
    code = torch.randint(0, 200, (1, L), generator=g).cuda()
    mel = torch.randn(1, 80, 2 * L, generator=g).cuda()
    spk = torch.rand(1, 256, generator=g).cuda()

    def run(v):
        with torch.no_grad():
            wav, pcm = v.forward_rows_precise(code, mel, spk)
        torch.cuda.synchronize()
        return {"wav": wav.clone(), "pcm": pcm.clone()}
    v = _vocoder(0)
    old = run(v)
    v.load_state_dict(tiny.synth(v, 1))
    new = run(v)
    assert _same(new, run(_vocoder(1))) and not _same(new, old)


def test_graph_cache_recaptures_after_a_reload(inputs):
    video, spk, _ = inputs
    m = _model(0)
    pipe = LipToSpeechPipeline(m, None)

    def fn(v, s):
        out = pipe.stage1_device(v, None, s)
        return tuple(out[k] for k in KEYS)
    cache = GraphCache(fn, state=lambda: state_epoch(m))
    for _ in range(2):
        got = [t.clone() for t in cache(video, spk)]
        torch.cuda.synchronize()
        assert cache.captures == 1 and len(cache.entries) == 1
        assert _same(dict(zip(KEYS, got)), _stage1(m, video, spk))
    m.load_state_dict(tiny.synth(m, 1))
    got = [t.clone() for t in cache(video, spk)]
    torch.cuda.synchronize()
    assert cache.captures == 2 and len(cache.entries) == 1
    assert _same(dict(zip(KEYS, got)), _stage1(_model(1), video, spk))


def test_stream_sub_batches_are_primed_again_after_a_reload(inputs):
    _, spk, u8 = inputs
    m, v = _model(0), _vocoder(0)
    pipe = LipToSpeechPipeline(m, v)
    keys = ("tokens", "lens", "mel", "wav", "pcm")

    def both():
        got = pipe.forward_device_u8_streams(u8, None, spk, streams=2)
        torch.cuda.synchronize()
        one = pipe.forward_device_u8(u8, None, spk)
        torch.cuda.synchronize()
        assert all(torch.equal(got[k], one[k]) for k in keys)
        return {k: got[k].clone() for k in keys}
    old = both()
    primed = len(pipe._shared_ready)
    both()
    assert len(pipe._shared_ready) == primed             # nothing moved: no second priming run
    m.load_state_dict(tiny.synth(m, 1))
    new = both()
    assert len(pipe._shared_ready) == primed + 1 and not _same(new, old)


def test_speaker_encoder_operands_follow_the_weights():
    enc = speaker_encoder.SpeakerEncoder()
    enc.load_state_dict(speaker_encoder.synthetic_state_dict(0))
    a = enc.pack("cuda")
    assert enc.pack(torch.device("cuda", torch.cuda.current_device())) is a
    sd = speaker_encoder.synthetic_state_dict(1)
    enc.load_state_dict(sd)
    b = enc.pack("cuda")
    assert b is not a
    assert torch.equal(b[1].cpu(), sd["linear.weight"].t()) and torch.equal(b[2].cpu(), sd["linear.bias"])
    assert not torch.equal(b[2], a[2])
