"""Text supervision on the MI355X: l2s_ctc_frames against torch fp32 softmax, l2s_ctc_beam_search against the CPU
restatement of ctcdecode (tests/_ctc_reference.py), the conformer's text head against the oracle conformer output, graph
capture, and the stage-1 CLI's pred_text files.
The edges of l2s_ctc_frames and l2s_ctc_repeat_labels are in the matrix of tests/test_glue_matrix_gpu.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import ops, weights  # noqa: E402
from tests import _ctc_reference as R  # noqa: E402
from tests.test_text_cpu import REVIVAL, revival_logits  # noqa: E402


def _frames_ref(logits, K):
    p = torch.softmax(logits.float(), -1)
    order = torch.from_numpy(np.argsort(-p.numpy(), axis=-1, kind="stable")[:, :K].copy())
    return p, order


@pytest.mark.parametrize("V,K", [(4000, 40), (39, 39), (4000, 64)])
def test_ctc_frames_matches_torch(V, K):
    g = torch.Generator().manual_seed(V + K)
    B, L = 3, 37
    ldl = -(-V // 4) * 4
    x = torch.randn(B * L, ldl, generator=g) * 3
    x[:, V:] = -3.0e38                                   # padded head columns (never read)
    x[5, 7] = x[5, 11] = x[5, :V].max() + 1.0            # exact tie at the top: first index wins
    x[9, :V] = 0.5                                       # a flat row: every class ties
    x[12, 100 % V] = x[12, 200 % V] = x[12, 300 % V]     # ties inside the top-K
    lens = torch.tensor([L, 20, 1], dtype=torch.int32)
    lab = torch.empty(B, L, dtype=torch.int32, device="cuda")
    tc = torch.empty(B, L, K, dtype=torch.int32, device="cuda")
    tl = torch.empty(B, L, K, device="cuda")
    ops.ctc_frames(x.cuda(), lab, tc, tl, B=B, L=L, V=V, K=K, ldl=ldl, lens=lens.cuda())
    torch.cuda.synchronize()
    lab, tc, tl = lab.cpu(), tc.cpu(), tl.cpu()
    p, order = _frames_ref(x[:, :V], K)
    for b in range(B):
        n = int(lens[b])
        rows = slice(b * L, b * L + n)
        assert torch.equal(lab[b, :n].long(), p[rows].argmax(-1)), b
        assert (lab[b, n:] == 0).all()
        for t in range(n):
            r = b * L + t
            assert set(tc[b, t].tolist()) == set(order[r].tolist()), (b, t)
            want = torch.log(p[r, tc[b, t].long()] + torch.finfo(torch.float32).tiny)
            assert (tl[b, t] - want).abs().max() < 1e-5
            assert (tl[b, t][1:] <= tl[b, t][:-1]).all()
        assert (tl[b, n:] == -torch.finfo(torch.float32).max).all()
    assert lab[0, 5].item() == 7
    assert lab[0, 9].item() == 0 and tc[0, 9].tolist() == list(range(K))


def _peaked(T, V, seed, scale=8.0, noise=1.0):
    r = np.random.default_rng(seed)
    x = r.normal(size=(T, V)).astype(np.float32) * noise
    t = 0
    while t < T:
        n = int(r.integers(1, 5))
        c = 0 if r.random() < 0.4 else int(r.integers(1, V))
        x[t:t + n, c] += scale
        t += n
    return x


def _gpu_beams(logits_list, beam, K, nbest=3):
    """Pad the clips to one batch, decode on the device; returns per clip [(labels, score)] of the nbest."""
    B = len(logits_list)
    L = max(x.shape[0] for x in logits_list)
    V = logits_list[0].shape[1]
    x = torch.zeros(B, L, V)
    for b, xb in enumerate(logits_list):
        x[b, : xb.shape[0]] = torch.from_numpy(xb)
    lens = torch.tensor([xb.shape[0] for xb in logits_list], dtype=torch.int32)
    d = ops.ctc_decode(x.view(B * L, V).cuda(), B=B, L=L, V=V, lens=lens.cuda(), len_mul=1, beam=beam, K=K, nbest=nbest)
    torch.cuda.synchronize()
    beams, blen, bsc = d["text_beams"].cpu(), d["text_lens"].cpu(), d["text_scores"].cpu()
    return [[(tuple(beams[b, h, : blen[b, h]].tolist()), float(bsc[b, h])) for h in range(beams.shape[1])] for b in range(B)]


def _check(got, ref, what, flat=False):
    ref = ref[: len(got)]
    for h, ((gl, gs), (rl, rs)) in enumerate(zip(got, ref)):
        if flat:   # only ranks the reference separates from both neighbours by > 1e-3
            gaps = [abs(rs - ref[j][1]) for j in (h - 1, h + 1) if 0 <= j < len(ref)]
            if min(gaps, default=1.0) <= 1e-3:
                continue
        assert gl == rl, f"{what} rank {h}: {gl} != {rl}"
        assert abs(gs - rs) <= 1e-4 * max(1.0, abs(rs)), f"{what} rank {h}: {gs} != {rs}"


@pytest.mark.parametrize("beam,K", [(30, 40), (64, 64)])
def test_ctc_beam_search_peaked_ragged(beam, K):
    V = 4000
    clips = [_peaked(120, V, 1), _peaked(77, V, 2), _peaked(9, V, 3)]
    got = _gpu_beams(clips, beam, K)
    for b, x in enumerate(clips):
        ref = R.beam_search(R.softmax32(x), beam=beam, cutoff_top_n=K)
        _check(got[b], ref, f"clip {b} beam {beam} K {K}")


def test_ctc_beam_search_long_clip():
    """T = 1200 frames (a 24-s clip at the unit rate)."""
    x = _peaked(1200, 4000, 7)
    got = _gpu_beams([x], 30, 40)
    ref = R.beam_search(R.softmax32(x), beam=30, cutoff_top_n=40)
    _check(got[0], ref, "T=1200")


def test_ctc_beam_search_revival_input():
    x = revival_logits()
    got = _gpu_beams([x], REVIVAL["beam"], REVIVAL["V"])
    ref = R.beam_search(R.softmax32(x), beam=REVIVAL["beam"], cutoff_top_n=REVIVAL["V"])
    bad = R.beam_search(R.softmax32(x), beam=REVIVAL["beam"], cutoff_top_n=REVIVAL["V"], fresh_ids=True)
    _check(got[0], ref, "revival")
    assert [lab for lab, _ in got[0]] != [lab for lab, _ in bad]        # the trie-less answer is not what the kernel gives


def test_ctc_beam_search_flat_and_short():
    r = np.random.default_rng(11)
    clips = [(r.normal(size=(40, 39)) * 0.5).astype(np.float32), (r.normal(size=(2, 39)) * 0.5).astype(np.float32)]
    got = _gpu_beams(clips, 30, 39)
    for b, x in enumerate(clips):
        ref = R.beam_search(R.softmax32(x), beam=30, cutoff_top_n=39)
        _check(got[b], ref, f"flat clip {b}", flat=True)
    # a beam that cannot exist: one frame, 2 classes -> 2 prefixes ("" and "1"); the third is empty with score FLT_MAX
    got = _gpu_beams([np.array([[0.3, 0.1]], np.float32)], 30, 2)[0]
    assert [lab for lab, _ in got] == [(), (1,), ()] and got[2][1] == float(R.FLT_MAX)


def _text_model(V_text, seed):
    from lip2speech_unit_amd.conformer import ConformerConfig
    from lip2speech_unit_amd.hubert import AVHubertConfig
    from lip2speech_unit_amd.model_avhubert import MultiTargetAVHubertEncoderModel
    model = MultiTargetAVHubertEncoderModel.build_model(
        dtype=ops.F16, w2v_cfg=AVHubertConfig(encoder_layers=2),
        conformer_cfg=ConformerConfig(conformer_layers=2, text_supervision=True))
    sd = weights.synth_state_dict(weights.spec_of(model), seed=seed)
    g = torch.Generator().manual_seed(seed)
    sd["conformer.text_classifier.classifier.weight"] = torch.randn(V_text, 512, generator=g) * 512 ** -0.5
    sd["conformer.text_classifier.classifier.bias"] = torch.randn(V_text, generator=g) * 0.1
    model.load_state_dict(sd)
    return model.cuda().eval(), sd


@pytest.mark.parametrize("V_text", [39, 4000])
def test_stage1_text_head_against_oracle(V_text):
    from lip2speech_unit_amd.pipeline import text_decode
    from oracle import stage1 as os1
    from tests.test_models_gpu import _frames
    model, sd = _text_model(V_text, 21)
    lens = [30, 17]
    B, T = len(lens), max(lens)
    video = _frames(B, T, 5)
    pad = torch.zeros(B, T, dtype=torch.bool)
    for b, n in enumerate(lens):
        pad[b, n:] = True
        video[b, :, n:] = 0
    spk = torch.rand(B, 256, generator=torch.Generator().manual_seed(3))
    m = model
    enc, dl, Bv, Tv = m.encoder.w2v_model.extract_rows(video.cuda(), pad.cuda())
    src16 = torch.empty(B * 2 * T, enc.shape[1], device="cuda", dtype=torch.float16)
    ops.repeat2_cast(enc, src16, B, T, enc.shape[1], ops.F16)
    _, _, y16 = m.conformer.forward_rows(src16, dl, B, 2 * T, spk.cuda(), len_mul=2)
    d = text_decode(m.conformer, y16, dl, B, 2 * T)
    torch.cuda.synchronize()
    W = sd["conformer.text_classifier.classifier.weight"].float()
    bias = sd["conformer.text_classifier.classifier.bias"].float()
    for b, n in enumerate(lens):
        taps = {}
        with torch.no_grad():
            os1.generate(sd, video[b:b + 1, :, :n], torch.zeros(1, n, dtype=torch.bool), spk[b:b + 1], enc_layers=2,
                         conf_layers=2, taps=taps)
        ref = taps["head_in"][0] @ W.t() + bias                                    # [2n, V_text]
        got = d["text_logits"][b, : 2 * n, :V_text].cpu()
        err = (got - ref).abs().max().item()
        assert err < 3e-2, err
        assert (d["text_logits"][b, :, V_text:] < -1e38).all()
        top2 = ref.topk(2, -1).values
        safe = (top2[:, 0] - top2[:, 1]) > 2 * err + 1e-3
        lab = d["text"][b].cpu().long()
        assert torch.equal(lab[: 2 * n][safe], ref.argmax(-1)[safe]), b
        assert int((~safe).sum()) <= 0.1 * 2 * n
        assert (lab[2 * n:] == 0).all()


def test_pipeline_text_beams_graph_replay_equals_eager():
    from lip2speech_unit_amd.pipeline import LipToSpeechPipeline
    from tests.test_models_gpu import _frames
    model, _ = _text_model(39, 22)
    pipe = LipToSpeechPipeline(model, vocoder=None)
    pipe.ctc_beam = True
    B, T = 2, 16
    video = _frames(B, T, 9).cuda()
    pad = torch.zeros(B, T, dtype=torch.bool)
    pad[1, 11:] = True
    pad = pad.cuda()
    spk = torch.rand(B, 256, generator=torch.Generator().manual_seed(4)).cuda()
    keys = ("tokens", "mel", "text", "text_beams", "text_lens", "text_scores", "text_logits")
    eager = {k: v.clone() for k, v in pipe.stage1_device(video, pad, spk).items() if k in keys}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pipe.stage1_device(video, pad, spk)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = pipe.stage1_device(video, pad, spk)
    g.replay()
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(out[k], eager[k]), k
    assert eager["text"].shape == (B, 2 * T) and eager["text_beams"].shape == (B, 3, 2 * T)
    assert (eager["text"][1, 22:] == 0).all()
    # the device beams equal the restatement run on the head's own logits
    for b, n in enumerate((2 * T, 22)):
        ref = R.beam_search(R.softmax32(eager["text_logits"][b, :n, :39].cpu().numpy()), beam=30, cutoff_top_n=39)
        got = [(tuple(eager["text_beams"][b, h, : int(eager["text_lens"][b, h])].tolist()), float(eager["text_scores"][b, h]))
               for h in range(3)]
        _check(got, ref, f"pipeline clip {b}", flat=True)


@pytest.mark.parametrize("beam", [False, True])
def test_stage1_cli_writes_pred_text(tmp_path, monkeypatch, beam):
    from lip2speech_unit_amd import inference as s1
    from tests._synth_dataset import make
    monkeypatch.setenv("TEXT_SUPERVISION", "1")
    if beam:
        monkeypatch.setenv("CTC_BS_DECODING", "1")
    else:
        monkeypatch.delenv("CTC_BS_DECODING", raising=False)
    lab = make(str(tmp_path / "ds"), frames=(12, 9, 5))
    out = str(tmp_path / "out")
    s1.main([f"common_eval.results_path={out}", f"override.data={lab}", f"override.label_dir={lab}", "synthetic_weights=true",
             "dataset.batch_size=2", "model.encoder_layers=2", "model.conformer_layers=2", "hipgraph=true"])
    for utt, T in zip(("test/spk0/00000", "test/spk1/00001", "test/spk0/00002"), (12, 9, 5)):
        lines = open(os.path.join(out, "pred_text", utt + ".txt")).read().split("\n")
        assert lines[-1] == ""
        lines = lines[:-1]
        if beam:
            assert len(lines) == 3
            for ln in lines:
                ids = [int(v) for v in ln.split()]
                assert len(ids) <= 2 * T and all(0 < v < 4000 for v in ids)
        else:
            assert len(lines) == 1
            ids = [int(v) for v in lines[0].split()]
            assert len(ids) == 2 * T and all(0 <= v < 4000 for v in ids)


def test_ctc_repeat_labels_matches_the_reference_fill():
    from lip2speech_unit_amd.data import repeat_text_labels
    g = torch.Generator().manual_seed(8)
    B, L = 3, 150
    x = torch.randint(1, 40, (B, L), generator=g, dtype=torch.int32)
    x[torch.rand(B, L, generator=g) < 0.6] = 0
    x[1, :70] = 0                                       # a long leading run of blanks
    lens = torch.tensor([75, 40, 1], dtype=torch.int32)       # x len_mul 2 = 150, 80, 2 frames
    y = torch.empty(B, L, dtype=torch.int32, device="cuda")
    ops.ctc_repeat_labels(x.cuda(), y, B=B, L=L, lens=lens.cuda(), len_mul=2)
    xi = x.cuda()
    ops.ctc_repeat_labels(xi, xi, B=B, L=L, lens=lens.cuda(), len_mul=2)           # in place
    y, xi = y.cpu(), xi.cpu()
    assert torch.equal(y, xi)
    for b in range(B):
        n = 2 * int(lens[b])
        assert y[b, :n].tolist() == repeat_text_labels(x[b, :n].tolist()), b
        assert (y[b, n:] == 0).all()


def _text_vocoder(dt, seed):
    from lip2speech_unit_amd.vocoder import AttrDict, MelCodeGenerator
    from tests.test_models_gpu import VOC_H
    h = AttrDict(dict(VOC_H, text_supervision=True, num_embeddings_text=4000, embedding_dim_text=589, model_in_dim=925))
    g = MelCodeGenerator(h, dtype=dt)
    g.load_state_dict(weights.synth_state_dict(weights.spec_of(g), seed=seed))
    g.remove_weight_norm()
    return g.cuda().eval()


@pytest.mark.parametrize("dt", [ops.F16, ops.BF16])
def test_vocoder_text_branch_vs_reference_fixture(golden_dir, dt):
    """models_multi_input.py with text supervision (4000 x 589, model_in_dim 925) run by tools/make_golden.py on two t_label rows
    with the same code / mel / speaker: both rows within the vocoder fixture tolerances, in 16-bit and at reference precision,
    and the two outputs differ from each other as the reference's do."""
    from tests.test_models_gpu import WAV_SNR_DB, WAV_TOL, _snr_db
    d = np.load(os.path.join(golden_dir, "vocoder_text.npz"))
    g = _text_vocoder(dt, int(d["seed"]))
    code, mel, spk = (torch.from_numpy(d[k]).cuda() for k in ("code", "mel", "spkr"))
    outs, outs_p = [], []
    for r in range(2):
        t = torch.from_numpy(d["t_label"][r:r + 1]).cuda()
        with torch.no_grad():
            wav, pcm = g.forward_rows(code, mel, spk, t_label=t)
            wav_p, pcm_p = g.forward_rows_precise(code, mel, spk, t_label=t)
        ref = torch.from_numpy(d["wav"][r, 0])
        err = (wav[0].cpu() - ref).abs().max().item()
        print(f"vocoder_text row {r}: 16-bit max |err| {err:.2e}, precise {(wav_p[0].cpu() - ref).abs().max().item():.2e}")
        assert err < WAV_TOL[dt] and _snr_db(ref.numpy(), wav[0].cpu().numpy()) > WAV_SNR_DB[dt]
        assert (wav_p[0].cpu() - ref).abs().max().item() < 4e-5
        assert np.abs(pcm_p[0].cpu().numpy().astype(np.int32) - d["pcm"][r].astype(np.int32)).max() <= 2
        outs.append(wav[0].cpu())
        outs_p.append(wav_p[0].cpu())
    ref_gap = float(np.abs(d["wav"][0, 0] - d["wav"][1, 0]).max())
    assert abs((outs[0] - outs[1]).abs().max().item() - ref_gap) < 2 * WAV_TOL[dt]
    assert abs((outs_p[0] - outs_p[1]).abs().max().item() - ref_gap) < 1e-4
    with pytest.raises(ValueError):                           # a text-supervised vocoder needs the labels
        g.forward_rows(code, mel, spk)


def test_fused_pipeline_with_text_equals_vocoder_fed_the_labels():
    """forward_device with a text head and a text-supervised vocoder equals the vocoder's forward_rows fed stage 1's framewise
    labels explicitly (REPEAT_TEXT_LABELS off and on); the whole path captured in one graph and replayed (beam decoding
    on) gives identical outputs."""
    from lip2speech_unit_amd.pipeline import LipToSpeechPipeline
    from tests.test_models_gpu import _frames
    model, _ = _text_model(4000, 23)
    voc = _text_vocoder(ops.F16, 24)
    B, T = 2, 12
    video = _frames(B, T, 19).cuda()
    pad = torch.zeros(B, T, dtype=torch.bool)
    pad[1, 8:] = True
    pad = pad.cuda()
    spk = torch.rand(B, 256, generator=torch.Generator().manual_seed(6)).cuda()
    for repeat in (False, True):
        pipe = LipToSpeechPipeline(model, voc)
        pipe.repeat_text = repeat
        out = pipe.forward_device(video, pad, spk)
        torch.cuda.synchronize()
        lens2 = (2 * out["lens"]).to(torch.int32)
        t = out["text"].clone()
        if repeat:
            from lip2speech_unit_amd.data import repeat_text_labels
            tc = t.cpu()
            for b in range(B):
                n = int(lens2[b])
                tc[b, :n] = torch.tensor(repeat_text_labels(tc[b, :n].tolist()), dtype=torch.int32)
            t = tc.cuda()
        code = (out["tokens"][:, : 2 * T].long() - 4).clamp(min=0)
        mel = out["mel"].transpose(1, 2).contiguous()
        wav, pcm = voc.forward_rows(code, mel, spk, lens2, t_label=t)
        torch.cuda.synchronize()
        assert torch.equal(out["pcm"], pcm), repeat
        assert (out["wav"] - wav).abs().max().item() == 0.0, repeat
    pipe = LipToSpeechPipeline(model, voc)
    pipe.ctc_beam = True
    keys = ("tokens", "text", "text_beams", "text_lens", "text_scores", "wav", "pcm")
    eager = {k: v.clone() for k, v in pipe.forward_device(video, pad, spk).items() if k in keys}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pipe.forward_device(video, pad, spk)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        cap = pipe.forward_device(video, pad, spk)
    gr.replay()
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(cap[k], eager[k]), k


def test_vocoder_cli_reads_text_labels(tmp_path, monkeypatch):
    import json
    from lip2speech_unit_amd import vocoder_inference as s2
    from tests._synth_dataset import make
    from tests.test_models_gpu import VOC_H
    lab = make(str(tmp_path / "ds"), frames=(12, 9, 5))
    rows = [[0, 3, 3, 0, 7] + [0] * 19, [2] + [0] * 17, [0, 0, 9] + [0] * 7]
    with open(os.path.join(lab, "test.txt"), "w") as f:
        f.write("\n".join(" ".join(str(x) for x in r) for r in rows) + "\n")
    cfg = str(tmp_path / "cfg.json")
    json.dump(dict(VOC_H, code_hop_size=320, mel_hop_size=160, sampling_rate=16000, num_embeddings_text=4000,
                   embedding_dim_text=589, model_in_dim=925), open(cfg, "w"))
    monkeypatch.setenv("TEXT_SUPERVISION", "1")
    out = []
    for i, r in enumerate((rows, [[5] * len(x) for x in rows])):
        with open(os.path.join(lab, "test.txt"), "w") as f:
            f.write("\n".join(" ".join(str(x) for x in row) for row in r) + "\n")
        d = str(tmp_path / f"out{i}")
        s2.main([cfg, os.path.join(lab, "test.tsv"), os.path.join(lab, "dict.unt.txt"), "--output_dir", d, "-n", "-1",
                 "--synthetic_weights"])
        from scipy.io import wavfile
        sr, wav = wavfile.read(os.path.join(d, "pred_wav", "spk1", "00001.wav"))
        assert sr == 16000 and wav.dtype == np.int16 and wav.shape[0] >= 17 * 320
        out.append(wav)
    assert not np.array_equal(out[0], out[1])                  # the label file reaches the vocoder
