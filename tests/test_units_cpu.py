"""Speech units from audio, the parts that need no GPU: the float64 restatement against HuggingFace's HuBERT, the quantiser
against the reference's ApplyKmeans, the frame-count formula against the committed label file, the host logic of the module and
its CLIs, the ABI entries' argument checks, and the decidability of the inputs the GPU id test uses."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import _units_reference as R

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_restatement_equals_huggingface_hubert(golden_dir):
    """(a) hidden_states[6] of transformers.HubertModel (an independent port of fairseq's module) on the same weights."""
    transformers = pytest.importorskip("transformers")
    case = R.shared_case(golden_dir)
    model = transformers.HubertModel(transformers.HubertConfig(num_hidden_layers=6)).double().eval()
    hf = R.to_huggingface({k: v.double() for k, v in case["sd"].items()})
    own = model.state_dict()
    assert set(own) - set(hf) == {"masked_spec_embed"} and not set(hf) - set(own)
    model.load_state_dict(hf, strict=False)
    wav = R.pcm_to_wave(case["pcm"]["c2"])
    with torch.no_grad():
        want = model(wav[None], output_hidden_states=True).hidden_states[6][0]
    got = case["feats"]["c2"]
    err = (got - want).abs().max().item()
    print(f"restatement vs transformers.HubertModel, layer 6, c2_pcm: max abs diff {err:.2e} (rms of the features {want.pow(2).mean().sqrt():.3f})")
    assert got.shape == want.shape == (63, 768) and err <= 1e-9


def test_init_follows_huggingface_rules():
    sd = R.init_weights(3, layers=1, perturb=False)
    assert not sd["post_extract_proj.bias"].any() and not sd["encoder.pos_conv.0.bias"].any()
    assert torch.equal(sd["layer_norm.weight"], torch.ones(512))
    assert abs(sd["encoder.layers.0.fc1.weight"].std().item() - 0.02) < 2e-4
    assert abs(sd["feature_extractor.conv_layers.1.0.weight"].std().item() - (2.0 / 1536) ** 0.5) < 2e-4
    v, g = sd["encoder.pos_conv.0.weight_v"], sd["encoder.pos_conv.0.weight_g"]
    assert torch.allclose(g, v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt(), rtol=1e-6)
    assert list(sd) == list(R.init_weights(3, layers=1)) and R.init_weights(3, layers=1)["post_extract_proj.bias"].any()


def test_quantiser_fixture_is_the_references_apply_kmeans(golden_dir):
    """(b) the recorded run of ApplyKmeans (tools/make_units_golden.py) against the restated formula, and the tool's inputs
    reproduce."""
    z = np.load(os.path.join(golden_dir, "units_kmeans.npz"))
    assert os.path.getsize(os.path.join(golden_dir, "units_kmeans.npz")) < 200 * 1024
    feats, cen, ids = z["features"], z["centers"], z["ids"]
    assert feats.shape == (130, 64) and cen.shape == (37, 64) and ids.shape == (130,) and ids.dtype == np.int32
    assert np.array_equal(R.kmeans_ids(feats, cen).numpy(), ids)
    assert np.array_equal(z["ids_f32"], ids)
    assert len(set(ids.tolist())) >= 30
    # the kernel's form of the distance (without the row-constant |x|^2) picks the same centre
    dev_ids, _, mask = R.decisive_rows(feats, cen)
    assert bool(mask.all()) and np.array_equal(dev_ids.numpy(), ids)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_units_golden as tool
    finally:
        sys.path.pop(0)
    f2, c2 = tool.make_case()
    assert np.array_equal(f2, feats) and np.array_equal(c2, cen)


def test_frame_counts_match_the_label_file(golden_dir):
    """(c) tokens per line of test.unt from the sample counts of test.tsv."""
    from lip2speech_unit_amd import speech_units
    d = os.path.join(golden_dir, "lrs3_sample")
    with open(os.path.join(d, "test.tsv")) as f:
        samples = [int(line.split("\t")[-1]) for line in f.read().splitlines()[1:]]
    with open(os.path.join(d, "test.unt")) as f:
        tokens = [len(line.split()) for line in f.read().splitlines()]
    assert len(samples) == len(tokens) >= 2
    for n, t in zip(samples, tokens):
        assert speech_units.num_frames(n) == R.frame_count(n) == t, (n, t)
    assert [speech_units.num_frames(n) for n in (68608, 39936, 20480, 57344, 24576)] == [214, 124, 63, 178, 76]
    assert speech_units.num_frames(400) == 1 and speech_units.num_frames(399) == 0 and speech_units.MIN_SAMPLES == 400


def test_state_dict_names_round_trip(golden_dir):
    """(d) fairseq's names, in and out; pre-training heads are accepted and ignored."""
    from lip2speech_unit_amd import speech_units
    sd = R.init_weights(0, layers=2)
    m = speech_units.HubertModel(speech_units.HubertConfig(encoder_layers=2))
    assert set(m.state_dict()) == set(sd)
    extra = dict(sd, mask_emb=torch.zeros(768), label_embs_concat=torch.zeros(504, 256))
    extra["final_proj.weight"], extra["final_proj.bias"] = torch.zeros(256, 768), torch.zeros(256)
    m.load_state_dict(extra)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "layer_norm.bias"})
    c = speech_units.HubertConfig()
    assert (c.encoder_layers, c.encoder_embed_dim, c.encoder_ffn_embed_dim, c.encoder_attention_heads) == (12, 768, 3072, 12)
    assert (c.conv_pos, c.conv_pos_groups, c.extractor_mode, c.layer_norm_first) == (128, 16, "default", False)


def test_unbuilt_options_are_named():
    from lip2speech_unit_amd import speech_units
    with pytest.raises(NotImplementedError, match="normalize"):
        speech_units.HubertModel(speech_units.HubertConfig(encoder_layers=1, normalize=True))
    with pytest.raises(NotImplementedError, match="extractor_mode"):
        speech_units.HubertModel(speech_units.HubertConfig(encoder_layers=1, extractor_mode="layer_norm"))


def test_load_hubert_reads_fairseq_layouts(tmp_path):
    from lip2speech_unit_amd import speech_units
    sd = R.init_weights(0, layers=1)
    new = tmp_path / "new.pt"
    torch.save({"model": dict(sd, mask_emb=torch.zeros(768)),
                "cfg": {"model": {"_name": "hubert", "encoder_layers": 1, "layer_norm_first": "False"}, "task": {"normalize": False}}}, new)
    m = speech_units.load_hubert(str(new))
    assert len(m.encoder.layers) == 1 and m.dtype == speech_units.ops.F32 and not m.training
    assert torch.equal(m.state_dict()["post_extract_proj.weight"], sd["post_extract_proj.weight"])
    old = tmp_path / "old.pt"
    import argparse
    torch.save({"model": sd, "args": argparse.Namespace(encoder_layers=1, extractor_mode="default", normalize=False)}, old)
    assert len(speech_units.load_hubert(str(old)).encoder.layers) == 1
    large = tmp_path / "large.pt"
    torch.save({"model": sd, "cfg": {"model": {"encoder_layers": 1}, "task": {"normalize": True}}}, large)
    with pytest.raises(NotImplementedError, match="normalize"):
        speech_units.load_hubert(str(large))
    bad = tmp_path / "bad.pt"
    torch.save({"generator": {}}, bad)
    with pytest.raises(ValueError):
        speech_units.load_hubert(str(bad))


def test_load_kmeans_reads_joblib_and_npy(tmp_path):
    joblib = pytest.importorskip("joblib")
    from lip2speech_unit_amd import speech_units
    cen = np.random.default_rng(0).standard_normal((7, 768))
    joblib.dump(types.SimpleNamespace(cluster_centers_=cen), tmp_path / "km.bin")
    np.save(tmp_path / "centers.npy", cen.astype(np.float32))
    a, b = speech_units.load_kmeans(str(tmp_path / "km.bin")), speech_units.load_kmeans(str(tmp_path / "centers.npy"))
    assert a.dtype == b.dtype == np.float32 and a.shape == (7, 768) and np.array_equal(a, b) and a.flags.c_contiguous
    np.save(tmp_path / "one.npy", cen[:1])
    with pytest.raises(ValueError):
        speech_units.load_kmeans(str(tmp_path / "one.npy"))
    hub = speech_units.HubertModel(speech_units.HubertConfig(encoder_layers=1))
    with pytest.raises(ValueError):
        speech_units.SpeechUnitExtractor(hub, cen[:, :64])
    with pytest.raises(ValueError):
        speech_units.SpeechUnitExtractor(hub, cen, layer=2)
    with pytest.raises(ValueError):
        speech_units.SpeechUnitExtractor(hub, cen, layer=1, dtype=speech_units.ops.F16)
    ex = speech_units.SpeechUnitExtractor(hub, cen, layer=1)
    assert torch.allclose(ex.cnorm.double(), torch.from_numpy(cen.astype(np.float32)).double().pow(2).sum(1), rtol=1e-6)
    with pytest.raises(speech_units.L2SError):
        ex.units(torch.zeros(1, 4000))                                   # a host tensor: there is no CPU path


def test_cli_argument_errors(tmp_path, capsys):
    from lip2speech_unit_amd import extract_units, vocoder_inference
    for argv in (["audio", "out.unt"], ["audio", "out.unt", "--hubert", "h.pt"],
                 [str(tmp_path), "out.unt", "--hubert", str(tmp_path / "none.pt"), "--kmeans", str(tmp_path / "none.bin")],
                 [str(tmp_path), "out.unt", "--hubert", "h", "--kmeans", "k", "--dtype", "f64"],
                 [str(tmp_path), "out.unt", "--hubert", "h", "--kmeans", "k", "--layer", "0"]):
        with pytest.raises(SystemExit) as e:
            extract_units.main(argv)
        assert e.value.code == 2, argv
    (tmp_path / "h.pt").write_bytes(b"x")
    (tmp_path / "k.bin").write_bytes(b"x")
    with pytest.raises(SystemExit) as e:
        extract_units.main([str(tmp_path / "missing"), "out.unt", "--hubert", str(tmp_path / "h.pt"), "--kmeans", str(tmp_path / "k.bin")])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        vocoder_inference.main(["cfg.json", "test.tsv", "dict.unt.txt", "--units_from_audio"])
    assert e.value.code == 2 and "--hubert" in capsys.readouterr().err
    # manifest order is kept, the root line is skipped
    man = tmp_path / "m.txt"
    man.write_text("/somewhere\nb/2.wav\t400\na/1.wav\t800\n")
    assert extract_units.list_clips("/r", str(man)) == ["/r/b/2.wav", "/r/a/1.wav"]


def test_extract_orders_batches_by_length_and_answers_in_input_order():
    from lip2speech_unit_amd import extract_units

    class Fake:
        def __init__(self):
            self.batches = []

        def units(self, wav, lens):
            self.batches.append(list(lens))
            return [np.full(n // 100, n) for n in lens]

    clips = [np.zeros(n, np.int16) for n in (700, 400, 900, 500, 600)]
    fake = Fake()
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self                      # the batching logic needs no device
    try:
        out = extract_units.extract(fake, clips, batch=2)
    finally:
        torch.Tensor.cuda = real_cuda
    assert fake.batches == [[400, 500], [600, 700], [900]]
    assert [int(o[0]) for o in out] == [700, 400, 900, 500, 600] and [len(o) for o in out] == [7, 4, 9, 5, 6]


def test_abi_entries_reject_bad_arguments_without_a_gpu():
    from lip2speech_unit_amd import _lib, ops
    lib = _lib.load()
    assert lib.l2s_abi_version() == 16 == _lib.ABI_VERSION
    assert lib.l2s_wave_stem_workspace(3, 512) == 3 * (16 + 1024) * 4 and lib.l2s_wave_stem_workspace(0, 512) == 0
    ok = dict(wav=0x1000, i16=0, ldw=8000, ns=None, B=3, S=8000, w=0x2000, g=0x3000, b=0x4000, eps=1e-5, out=0x5000, ldo=512, T=1599,
              C=512, ws=0x6000, wsb=3 * 1040 * 4, dtype=0, stream=None)

    def stem(**kw):
        a = dict(ok, **kw)
        return lib.l2s_wave_stem(a["wav"], a["i16"], a["ldw"], a["ns"], a["B"], a["S"], a["w"], a["g"], a["b"], a["eps"], a["out"], a["ldo"],
                                 a["T"], a["C"], a["ws"], a["wsb"], a["dtype"], a["stream"])
    for name in ("wav", "w", "g", "b", "out", "ws"):
        assert stem(**{name: None}) == -1, name
    assert stem(dtype=3) == -1
    assert stem(B=0) == -2 and stem(ldw=7999) == -2 and stem(ldo=511) == -2 and stem(T=1598) == -2 and stem(wsb=100) == -2
    assert stem(C=256, ldo=256) == -4 and stem(B=70000, wsb=1 << 40) == -4
    assert stem(wav=0x1002) == -3 and stem(wav=0x1001, i16=1) == -3 and stem(out=0x5002) == -3 and stem(out=0x5004, dtype=2) == -3
    okk = dict(x=0x1000, ldx=768, cen=0x2000, cn=0x3000, lens=None, len_mul=1, B=2, T=65, D=768, K=200, ids=0x4000, best2=None, stream=None)

    def km(**kw):
        a = dict(okk, **kw)
        return lib.l2s_kmeans_assign(a["x"], a["ldx"], a["cen"], a["cn"], a["lens"], a["len_mul"], a["B"], a["T"], a["D"], a["K"], a["ids"],
                                     a["best2"], a["stream"])
    for name in ("x", "cen", "cn", "ids"):
        assert km(**{name: None}) == -1, name
    assert km(lens=0x7000, len_mul=0) == -1
    assert km(B=0) == -2 and km(T=0) == -2 and km(ldx=767) == -2 and km(K=0) == -2
    assert km(D=40, ldx=40) == -4 and km(D=1056, ldx=1056) == -4 and km(K=1) == -4 and km(K=1025) == -4
    assert km(x=0x1004) == -3 and km(cen=0x2008) == -3 and km(ldx=770) == -3 and km(ids=0x4002) == -3
    for name in ("wave_stem", "kmeans_assign"):
        assert ops.ENTRY_OF[name] == "l2s_" + name and hasattr(torch.ops.lip2speech, name)
    assert "l2s_wave_stem_workspace" in ops.HOST_QUERIES
    with pytest.raises(ops.L2SError):
        ops.kmeans_assign(torch.zeros(4, 32), torch.zeros(2, 32), torch.zeros(2), torch.zeros(4, dtype=torch.int32), B=1, T=4, D=32, K=2)


def test_post_ln_encoder_is_accepted_and_pre_ln_refuses_output_layer():
    from lip2speech_unit_amd import ops, speech_units
    from lip2speech_unit_amd.hubert import AVHubertConfig, TransformerEncoder
    enc = TransformerEncoder(speech_units.HubertConfig(encoder_layers=2), dtype=ops.F32)
    assert len(enc.layers) == 2 and not enc.cfg.layer_norm_first
    pre = TransformerEncoder(AVHubertConfig(encoder_layers=1, encoder_embed_dim=128, encoder_ffn_embed_dim=256, encoder_attention_heads=2))
    with pytest.raises(NotImplementedError):
        pre.forward_rows(torch.zeros(4, 128), torch.zeros(4, 128), None, 1, 4, output_layer=1)


def test_kernel_test_inputs_are_decidable_in_float64():
    """The quantiser cases of tests/test_units_kernels_gpu.py: at most 1 % of rows under the fp32-rounding gap, by the reference alone."""
    for D, K in ((768, 200), (32, 2), (1024, 1000), (768, 37)):
        x, c = R.kmeans_case(D, K)
        ids, best2, mask = R.decisive_rows(x, c)
        assert x.shape == (130, D) and c.shape == (K, D)
        assert (~mask).double().mean().item() <= 0.01, (D, K)
        assert torch.equal(ids[mask], R.kmeans_ids(x, c)[mask])      # with or without the row-constant |x|^2


def test_id_test_inputs_are_decidable(golden_dir):
    """(e) r_t = min_{j != id} (d_j - d_id) / (2 |c_j - c_id| |x_t|), the relative feature error frame t tolerates: none at or
    under 1e-4 and at most 10 % at or under 1e-3, for c2_pcm and c4_pcm against 100 centres drawn from c1_pcm's frames."""
    case = R.shared_case(golden_dir)
    assert case["centers"].shape == (100, 768) and case["centers"].dtype == torch.float32
    for clip, frames in (("c2", 63), ("c4", 76)):
        x = case["feats"][clip]
        ids, r = R.flip_margin(x, case["centers"])
        share = (r <= 1e-3).double().mean().item()
        print(f"{clip}_pcm: {x.shape[0]} frames, min r_t {r.min().item():.2e}, share with r_t <= 1e-3 {100 * share:.1f} %, "
              f"{ids.unique().numel()} distinct ids")
        assert x.shape == (frames, 768)
        assert not bool((r <= 1e-4).any())
        assert share <= 0.10
        assert ids.unique().numel() >= 30
        assert torch.equal(ids, R.kmeans_ids(x, case["centers"]))
