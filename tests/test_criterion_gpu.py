"""The `multi_target` criterion on the device (csrc/criterion.hip, criterion.py, validate.py) against float64: the golden file the
reference's own program wrote, and torch on the CPU for seeded larger shapes.  The product's output is never the yardstick.

Gate 1, for every per-clip quantity q:  |q_device - q_fp64| <= 4 * max(u, 2^-23 * S_abs)  with u = |fp32 CPU evaluation - fp64|
and S_abs the fp64 sum of the absolute values of the terms q accumulates (the sums here have positive terms only, so S_abs = |q|;
for CTC S_abs = sum_t |logsumexp_t| + |q|).  The worst ratio  |q_device - q_fp64| / max(u, 2^-23 S_abs)  is printed per test."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lip2speech_unit_amd import ops, weights
from tests import _criterion_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "criterion.npz")
PAD = 1
FACTOR = 4.0


def _ratio(dev, f64, f32, s_abs):
    """Worst |dev - f64| / max(|f32 - f64|, 2^-23 S_abs) over the clips; a clip whose unit is 0 must match exactly."""
    dev, f64, f32, s_abs = (np.asarray(torch.as_tensor(x).double().cpu() if torch.is_tensor(x) else x, np.float64).reshape(-1)
                            for x in (dev, f64, f32, s_abs))
    unit = np.maximum(np.abs(f32 - f64), 2.0 ** -23 * np.abs(s_abs))
    err = np.abs(dev - f64)
    assert (err[unit == 0] == 0).all(), (dev[unit == 0], f64[unit == 0])
    return float((err[unit > 0] / unit[unit > 0]).max()) if (unit > 0).any() else 0.0


def _gate(name, dev, f64, f32, s_abs=None):
    r = _ratio(dev, f64, f32, f64 if s_abs is None else s_abs)
    print(f"gate {name}: worst ratio {r:.3f} (limit {FACTOR:g})")
    assert r <= FACTOR, (name, r)
    return r


def _i32(x):
    return torch.as_tensor(x).to(torch.int32).cuda()


def unit_ce(logits, target, lens):
    B, T2, V = logits.shape
    d = logits.cuda().contiguous()
    out = (torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, device="cuda", dtype=torch.int32),
           torch.empty(B, device="cuda", dtype=torch.int32))
    tgt = _i32(target).contiguous()
    ops.unit_ce(d, tgt, *out, B=B, T2=T2, V=V, lens=_i32(lens), len_mul=2, pad_idx=PAD)
    return [o.cpu() for o in out]


def mel_sums(pred, targ, lens):
    B, Tp, C = pred.shape
    out = (torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, device="cuda"),
           torch.empty(B, device="cuda", dtype=torch.int32))
    crop = min(4 * int(max(lens)), Tp, targ.shape[1])
    ops.mel_l1_sc(pred.cuda().contiguous(), targ.cuda().contiguous(), *out, B=B, Tm_pred=Tp, Tm_targ=targ.shape[1], crop_len=crop,
                  lens=_i32(lens), len_mul=4, n_mels=C)
    return [o.cpu() for o in out]


def ctc(text, labels, label_lens, lens, blank=0):
    """text [B, L, V] fp32."""
    B, L, V = text.shape
    tl = _i32(label_lens)
    offs = (torch.cumsum(tl, 0, dtype=torch.int32) - tl).contiguous()
    s_max = int(max(label_lens)) if len(label_lens) else 0
    work = torch.empty(ops.ctc_loss_workspace_bytes(B, L, s_max) // 4, device="cuda")
    nll = torch.empty(B, device="cuda")
    ops.ctc_loss(text.cuda().contiguous(), _i32(labels), tl, offs, work, nll, B=B, L=L, V=V, S_max=s_max, blank=blank, lens=_i32(lens),
                 len_mul=2)
    return nll.cpu()


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLDEN))
    net = {k: torch.from_numpy(g[k]) for k in ("encoder_out", "encoder_out_mel", "encoder_out_text")}
    sample = {k: torch.from_numpy(g[k]) for k in ("target", "mel", "input_lengths", "text_labels", "text_labels_lengths", "padding_mask")}
    sample["ntokens"] = int(g["ntokens"])
    return g, net, sample


# ---- 1. kernel parity --------------------------------------------------------------------------------------------------------------
def test_kernels_against_the_golden_file(gold):
    g, net, s = gold
    lens = s["input_lengths"]
    kw = dict(pad=PAD, label_smoothing=0.1, mel_weight=10.0, sentence_avg=False, text_supervision=True)
    _, c64 = R.forward(net, s, **kw)
    _, c32 = R.forward(net, s, dtype=torch.float32, **kw)
    nll, smooth, ok, n = unit_ce(net["encoder_out"], s["target"], lens)
    # the stored per-clip values of the reference's own runs are the yardstick where the file has them ...
    _gate("golden nll", nll, g["f64_sa0_clip_nll_loss"], g["f32_sa0_clip_nll_loss"])
    assert ok.tolist() == g["f64_sa0_clip_n_correct"].astype(int).tolist() and n.tolist() == g["f64_sa0_clip_total"].astype(int).tolist()
    # ... and the float64 restatement (held to the file at 1e-12 by test_criterion_reference_cpu.py) for the sums it does not log
    _gate("golden smooth", smooth, c64["smooth"], c32["smooth"])
    l1, sq, tsq, rows = mel_sums(net["encoder_out_mel"], s["mel"], lens)
    for name, got in (("l1", l1), ("sq", sq), ("tsq", tsq)):
        _gate("golden " + name, got, c64[name], c32[name])
    assert rows.tolist() == c64["rows"].tolist()
    nllc = ctc(net["encoder_out_text"].transpose(0, 1), s["text_labels"], s["text_labels_lengths"].tolist(), lens)
    _gate("golden ctc", nllc, g["f64_sa0_clip_ctc_loss"], g["f32_sa0_clip_ctc_loss"], c64["lse_abs"].numpy() + g["f64_sa0_clip_ctc_loss"])
    tl, fr = g["text_labels_lengths"], g["input_lengths"]
    assert (nllc.numpy()[tl > 2 * fr] == 0).all()                     # no alignment -> 0 (zero_infinity)


@pytest.fixture(scope="module")
def unit_case():
    """640 clips x 200 unit frames x 204 classes, mixed lengths, top-two gap of every row >= 1e-3."""
    g = torch.Generator().manual_seed(7)
    B, T, V = 640, 100, 204
    logits = torch.randn(B, 2 * T, V, generator=g) * 2.0
    top = logits.topk(2, -1)
    bump = (top.values[..., 0] - top.values[..., 1]) < 4e-3
    logits.scatter_add_(-1, top.indices[..., :1], (bump.float() * 1.6e-2).unsqueeze(-1))
    lens = torch.randint(20, T + 1, (B,), generator=g)
    lens[0], lens[1] = T, 1
    target = torch.randint(4, V, (B, 2 * T), generator=g)
    hit = torch.rand(B, 2 * T, generator=g) < 0.5
    target = torch.where(hit, logits.argmax(-1), target)
    nlab = (2 * lens - torch.randint(0, 3, (B,), generator=g)).clamp(min=1)       # a few labels short of 2 * frames, or equal
    target[torch.arange(2 * T)[None, :] >= nlab[:, None]] = PAD
    target[2, 5] = PAD                                                            # a pad inside the labels
    return logits, target, lens


def test_unit_ce_at_batch_scale_and_determinism(unit_case):
    logits, target, lens = unit_case
    c64 = R.unit_ce_per_clip(logits, target, lens, PAD, torch.float64)
    c32 = R.unit_ce_per_clip(logits, target, lens, PAD, torch.float32)
    assert R.top2_gap(logits, c64["mask"]) >= 1e-3
    assert torch.equal(c64["n_correct"], c32["n_correct"])
    got = unit_ce(logits, target, lens)
    _gate("unit nll 640x200x204", got[0], c64["nll"], c32["nll"])
    _gate("unit smooth 640x200x204", got[1], c64["smooth"], c32["smooth"])
    assert torch.equal(got[2].long(), c64["n_correct"]) and torch.equal(got[3].long(), c64["n_tok"])
    assert 0.3 < float(c64["n_correct"].sum()) / float(c64["n_tok"].sum()) < 0.7
    again = unit_ce(logits, target, lens)                                          # 3. determinism: identical bytes
    for a, b in zip(got, again):
        assert a.numpy().tobytes() == b.numpy().tobytes()


def test_unit_ce_odd_class_counts_and_strides():
    """V outside the float4 path (odd, and a row stride that breaks 16-byte alignment), V = 4096 (the cap), ldt < T2."""
    g = torch.Generator().manual_seed(11)
    for V, ld, T2, ldt in ((203, 203, 9, 9), (204, 206, 9, 7), (4096, 4096, 5, 5), (5, 8, 70, 70)):
        B = 3
        buf = torch.randn(B * T2, ld, generator=g) * 3
        logits = buf[:, :V].reshape(B, T2, V)
        target = torch.randint(0, V, (B, ldt), generator=g)
        target[target == PAD] = 0
        target[1, -1] = PAD
        lens = torch.tensor([T2, (T2 + 1) // 2, 1])
        c64 = R.unit_ce_per_clip(logits, target, lens, PAD, torch.float64)
        c32 = R.unit_ce_per_clip(logits, target, lens, PAD, torch.float32)
        out = (torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, device="cuda", dtype=torch.int32),
               torch.empty(B, device="cuda", dtype=torch.int32))
        ops.unit_ce(buf.cuda()[:, :V], _i32(target), *out, B=B, T2=T2, V=V, ldl=ld, lens=_i32(lens), len_mul=2, pad_idx=PAD)
        _gate(f"unit nll V={V} ld={ld}", out[0], c64["nll"], c32["nll"])
        _gate(f"unit smooth V={V} ld={ld}", out[1], c64["smooth"], c32["smooth"])
        assert torch.equal(out[3].cpu().long(), c64["n_tok"])
        if R.top2_gap(logits, c64["mask"]) >= 1e-6:
            assert torch.equal(out[2].cpu().long(), c64["n_correct"])
    # first index on ties
    logits = torch.zeros(1, 2, 8)
    logits[0, 0, [3, 6]] = 1.0
    logits[0, 1, [7, 2]] = 2.0
    got = unit_ce(logits, torch.tensor([[3, 7]]), [1])
    assert got[2].tolist() == [1] and got[3].tolist() == [2]                       # row 0: argmax 3 = target; row 1: argmax 2 != 7
    with pytest.raises(ops.L2SError, match="EUNSUPPORTED"):
        unit_ce(torch.zeros(1, 2, 4097), torch.zeros(1, 2), [1])


def test_mel_sums_at_batch_scale():
    g = torch.Generator().manual_seed(13)
    B, T = 96, 200
    lens = torch.randint(5, T + 1, (B,), generator=g)
    lens[0] = T
    pred = torch.randn(B, 4 * T, 80, generator=g) * 2 - 5
    targ = torch.zeros(B, 4 * T + 2, 80)
    for b in range(B):
        n = int(4 * lens[b]) + int(torch.randint(-3, 3, (1,), generator=g))       # a target shorter or longer than 4 * frames
        targ[b, :n] = torch.randn(n, 80, generator=g) * 2 - 5
    c64, c32 = R.mel_sums_per_clip(pred, targ, lens), R.mel_sums_per_clip(pred, targ, lens, torch.float32)
    got = mel_sums(pred, targ, lens)
    for name, q in zip(("l1", "sq", "tsq"), got):
        _gate(f"mel {name} 96x800x80", q, c64[name], c32[name])
    assert torch.equal(got[3].long(), c64["rows"])
    again = mel_sums(pred, targ, lens)
    assert all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(got, again))
    # a prediction shorter than the target and than 4 * frames crops both (criterion.py:67); odd channel count = scalar path
    p2, t2 = pred[:3, :50, :79].contiguous(), targ[:3, :61, :79].contiguous()
    c64, c32 = R.mel_sums_per_clip(p2, t2, lens[:3]), R.mel_sums_per_clip(p2, t2, lens[:3], torch.float32)
    got = mel_sums(p2, t2, lens[:3])
    for name, q in zip(("l1", "sq", "tsq"), got):
        _gate(f"mel {name} cropped, 79 wide", q, c64[name], c32[name])
    assert got[3].tolist() == c64["rows"].tolist() == [min(50, 4 * int(n)) for n in lens[:3]]


@pytest.fixture(scope="module")
def text_case():
    """V = 4000 text classes, up to 1 200 frames, targets with repeats, the 511-label cap, an empty and an impossible target."""
    g = torch.Generator().manual_seed(17)
    frames = [600, 450, 300, 40, 3]
    B, L, V = len(frames), 1200, 4000
    text = torch.randn(B, L, V, generator=g) * 1.5
    counts = [120, 511, 0, 60, 7]                                                 # clip 4: 7 labels over 6 frames -> 0
    labels = []
    for n in counts:
        lab = torch.randint(1, V, (n,), generator=g)
        if n > 4:
            lab[1::5] = lab[0:-1:5][: len(lab[1::5])]                              # repeats: a blank is needed between them
        labels.append(lab)
    for b, lab in enumerate(labels):                                              # make the labels likely: a loss of usable size
        for j, c in enumerate(lab.tolist()):
            t = j * (2 * frames[b]) // max(len(lab), 1)
            text[b, t, c] += 6.0
    return text, labels, frames


def _torch_ctc(text, labels, frames, dtype):
    lp = F.log_softmax(text.to(dtype), -1).transpose(0, 1)
    il = torch.tensor([min(2 * f, text.shape[1]) for f in frames])
    return F.ctc_loss(lp, torch.cat(labels).long(), il, torch.tensor([len(x) for x in labels]), blank=0, reduction="none",
                      zero_infinity=True)


def test_ctc_at_v4000_l1200(text_case):
    text, labels, frames = text_case
    n64, n32 = _torch_ctc(text, labels, frames, torch.float64), _torch_ctc(text, labels, frames, torch.float32)
    lse = torch.logsumexp(text.double(), -1).abs()
    s_abs = torch.stack([lse[b, : 2 * f].sum() for b, f in enumerate(frames)]) + n64.abs()
    got = ctc(text, torch.cat(labels), [len(x) for x in labels], frames)
    assert n64[4] == 0 and got[4] == 0 and n64[2] > 0 and n64[1] > 0
    _gate("ctc V=4000 L=1200", got, n64, n32, s_abs)
    again = ctc(text, torch.cat(labels), [len(x) for x in labels], frames)
    assert got.numpy().tobytes() == again.numpy().tobytes()
    with pytest.raises(ops.L2SError, match="unsupported size"):
        ops.ctc_loss_workspace_bytes(2, 100, 512)
    assert ops.ctc_loss_workspace_bytes(2, 100, 511) == 2 * 100 * 512 * 4


# ---- 5. CTC edge cases, exactly as torch ---------------------------------------------------------------------------------------------
def test_ctc_edge_cases_against_torch():
    g = torch.Generator().manual_seed(19)
    V, L = 50, 12
    six = [3, 4, 5, 6, 7, 8]
    # (labels, video frames): the clip has 2 * frames CTC inputs; S labels with r adjacent repeats need S + r of them
    cases = [([], 6), ([], 1), ([7], 1), ([7, 7], 2), ([7, 7], 1), ([7, 7, 7], 3), ([7, 7, 7], 2), (six, 2), (six, 3),
             ([9, 9, 4, 4, 9], 4), ([9, 9, 4, 4, 9], 3), ([5], 6)]
    labels = [torch.tensor(c[0], dtype=torch.long) for c in cases]
    frames = [c[1] for c in cases]                                                # 2 * frames CTC inputs each
    text = torch.randn(len(cases), L, V, generator=g) * 2
    for blank in (0, 49):
        labs = [torch.where(x == blank, torch.tensor(1), x) for x in labels]
        lp64 = F.log_softmax(text.double(), -1).transpose(0, 1)
        il, tl = torch.tensor([2 * f for f in frames]), torch.tensor([len(x) for x in labs])
        n64 = F.ctc_loss(lp64, torch.cat(labs), il, tl, blank=blank, reduction="none", zero_infinity=True)
        n32 = F.ctc_loss(F.log_softmax(text, -1).transpose(0, 1), torch.cat(labs), il, tl, blank=blank, reduction="none", zero_infinity=True)
        raw = F.ctc_loss(lp64, torch.cat(labs), il, tl, blank=blank, reduction="none", zero_infinity=False)
        got = ctc(text, torch.cat(labs), tl.tolist(), frames, blank=blank)
        assert (got[torch.isinf(raw)] == 0).all() and int(torch.isinf(raw).sum()) == 4       # the four clips with too few inputs
        lse = torch.logsumexp(text.double(), -1).abs()
        s_abs = torch.stack([lse[b, : 2 * f].sum() for b, f in enumerate(frames)]) + n64.abs()
        _gate(f"ctc edge cases blank={blank}", got, n64, n32, s_abs)
        mine = [R.ctc_alpha_nll(lp64[: 2 * f, b].numpy(), labs[b].tolist(), blank) for b, f in enumerate(frames)]
        assert np.allclose([0.0 if np.isinf(x) else x for x in mine], n64.numpy(), rtol=1e-12, atol=0)


# ---- 2. clip-alone -------------------------------------------------------------------------------------------------------------------
def test_clip_alone_bit_for_bit(gold, text_case):
    """Each clip's partials from a padded batch of mixed lengths equal those of the clip run alone (B = 1), byte for byte."""
    _, net, s = gold
    lens = s["input_lengths"].tolist()
    tl = s["text_labels_lengths"].tolist()
    off = np.concatenate([[0], np.cumsum(tl)])
    text = net["encoder_out_text"].transpose(0, 1).contiguous()
    batch = (unit_ce(net["encoder_out"], s["target"], lens) + mel_sums(net["encoder_out_mel"], s["mel"], lens)
             + [ctc(text, s["text_labels"], tl, lens)])
    for b in range(len(lens)):
        alone = (unit_ce(net["encoder_out"][b:b + 1], s["target"][b:b + 1], lens[b:b + 1])
                 + mel_sums(net["encoder_out_mel"][b:b + 1], s["mel"][b:b + 1], lens[b:b + 1])
                 + [ctc(text[b:b + 1], s["text_labels"][off[b]:off[b + 1]], tl[b:b + 1], lens[b:b + 1])])
        for q, a in zip(batch, alone):
            assert q[b:b + 1].numpy().tobytes() == a.numpy().tobytes(), b
    # the V = 4000 case: alone, a clip also gets a workspace sized for its own label count
    text, labels, frames = text_case
    batch = ctc(text, torch.cat(labels), [len(x) for x in labels], frames)
    for b in (0, 3):
        alone = ctc(text[b:b + 1, : 2 * frames[b]], labels[b], [len(labels[b])], frames[b:b + 1])
        assert batch[b:b + 1].numpy().tobytes() == alone.numpy().tobytes(), b


# ---- 4. graph capture ----------------------------------------------------------------------------------------------------------------
class _Task:
    class _D:
        def pad(self):
            return PAD
    target_dictionary = _D()

    def __init__(self, text):
        self.cfg = {"text_supervision": text}


class _FixedModel(torch.nn.Module):
    """Hands out a net_output it was given (the criterion is what is captured here; the models' own captures have their tests)."""

    def __init__(self, net_output):
        super().__init__()
        self.net_output = net_output

    def forward(self, **net_input):
        return dict(self.net_output)


def _device_sample(net, s, lengths_on_device):
    dev = "cuda"
    sample = {"net_input": {"padding_mask": s["padding_mask"].to(dev)}, "target": s["target"].to(dev), "mel": s["mel"].to(dev),
              "ntokens": s["ntokens"], "input_lengths": s["input_lengths"], "text_labels": s["text_labels"].to(dev),
              "text_labels_lengths": s["text_labels_lengths"].to(dev) if lengths_on_device else s["text_labels_lengths"]}
    return {k: v.to(dev) for k, v in net.items()}, sample


@pytest.mark.parametrize("sentence_avg", [False, True])
def test_forward_against_the_golden_file_and_graph_replay(gold, sentence_avg):
    from lip2speech_unit_amd.criterion import MultiTargetCriterion
    g, net, s = gold
    crit = MultiTargetCriterion(_Task(True), sentence_avg, 0.1, 10.0, report_accuracy=True)
    dnet, sample = _device_sample(net, s, lengths_on_device=False)
    loss, sample_size, log = crit(_FixedModel(dnet), sample)
    assert loss.dim() == 0 and loss.is_cuda and all(log[k].is_cuda and log[k].dim() == 0 for k in ("loss", "nll_loss", "mel_loss", "ctc_loss"))
    tag = f"sa{int(sentence_avg)}_"
    kw = dict(pad=PAD, label_smoothing=0.1, mel_weight=10.0, sentence_avg=sentence_avg, text_supervision=True)
    _, c64 = R.forward(net, s, **kw)
    s_abs = {"loss": float(g["f64_" + tag + "loss"]) + float(c64["lse_abs"].sum()), "nll_loss": None, "mel_loss": None,
             "ctc_loss": float(g["f64_" + tag + "ctc_loss"]) + float(c64["lse_abs"].sum())}
    for k in ("loss", "nll_loss", "mel_loss", "ctc_loss"):
        _gate(f"forward {k} sentence_avg={sentence_avg}", log[k], g["f64_" + tag + k], g["f32_" + tag + k], s_abs[k])
    for k in ("ntokens", "nsentences", "sample_size", "n_correct", "total"):
        assert int(log[k]) == int(g["f64_" + tag + k]), k
    assert sample_size == int(g["f64_" + tag + "sample_size"]) and torch.equal(loss, log["loss"])
    # per clip against the reference's one-clip runs
    part = crit.last_partials
    _gate("forward per-clip mel_loss", part["mel_loss"], g["f64_" + tag + "clip_mel_loss"], g["f32_" + tag + "clip_mel_loss"])
    _gate("forward per-clip loss", part["loss"], g["f64_" + tag + "clip_loss"], g["f32_" + tag + "clip_loss"],
          g["f64_" + tag + "clip_loss"] + c64["lse_abs"].numpy())
    # captured and replayed: everything the call reads is on the device (the lengths too), nothing syncs
    dnet, sample = _device_sample(net, s, lengths_on_device=True)
    model = _FixedModel(dnet)
    eager = crit(model, sample)[2]
    eager = {k: v.clone() for k, v in eager.items() if torch.is_tensor(v)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        crit(model, sample)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = crit(model, sample)[2]
    for v in cap.values():
        if torch.is_tensor(v):
            v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert set(eager) == {"loss", "nll_loss", "mel_loss", "ctc_loss", "n_correct", "total"}
    for k, v in eager.items():
        assert v.cpu().numpy().tobytes() == cap[k].cpu().numpy().tobytes(), k
    assert torch.equal(eager["loss"], log["loss"])                      # host or device lengths: the same result


# ---- 6. model level ------------------------------------------------------------------------------------------------------------------
class _Recorder(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, **kw):
        self.out = self.model(**kw)
        return self.out


def _sample_for(B, T, lens, V, seed, text_classes=0):
    from tests.test_models_gpu import _frames
    g = torch.Generator().manual_seed(seed)
    video = _frames(B, T, seed)
    pm = torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]
    video[pm[:, None, :, None, None].expand_as(video)] = 0
    counts = [2 * n - (b % 2) for b, n in enumerate(lens)]
    target = torch.full((B, max(counts)), PAD, dtype=torch.long)
    for b, n in enumerate(counts):
        target[b, :n] = torch.randint(4, V, (n,), generator=g)
    mel = torch.zeros(B, 4 * T + 2, 80)
    for b, n in enumerate(lens):
        mel[b, : 4 * n + 2 - 3 * (b % 2)] = -11.5 + 11.4 * torch.rand(4 * n + 2 - 3 * (b % 2), 80, generator=g)
    s = {"net_input": {"source": {"audio": None, "video": video.cuda()}, "padding_mask": pm.cuda(),
                       "spk_emb": torch.rand(B, 256, generator=g).cuda()},
         "target": target.cuda(), "ntokens": int(sum(counts)), "mel": mel.cuda(), "input_lengths": torch.tensor(lens, dtype=torch.int32)}
    if text_classes:
        tl = [min(5 + 3 * b, 2 * n + 2) for b, n in enumerate(lens)]
        labs = [torch.randint(1, text_classes, (n,), generator=g) for n in tl]
        labs[0][1] = labs[0][0]
        s["text_labels"] = torch.cat(labs).int().cuda()
        s["text_labels_lengths"] = torch.tensor(tl, dtype=torch.int32)
    return s


def _check_valid_step(model, text, V_text=0, name=""):
    from lip2speech_unit_amd.criterion import MultiTargetCriterion
    from lip2speech_unit_amd.task import Lip2SpeechTask, UnitDictionary, decode_config
    task = Lip2SpeechTask(decode_config(), dictionary=UnitDictionary([str(i) for i in range(200)]))
    task.cfg.text_supervision = text
    crit = task.build_criterion({"_name": "multi_target", "label_smoothing": 0.1, "mel_weight": 10, "report_accuracy": True})
    assert type(crit) is MultiTargetCriterion and crit.text_supervision == text
    lens = [9, 4, 7]
    sample = _sample_for(3, 9, lens, 204, 31, text_classes=V_text)
    rec = _Recorder(model)
    loss, sample_size, log = task.valid_step(sample, rec, crit)
    assert sample_size == sample["ntokens"] and not loss.requires_grad
    net = {k: v.detach().float().cpu() for k, v in rec.out.items() if k.startswith("encoder_out") and v is not None}
    host = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in sample.items() if k != "net_input"}
    kw = dict(pad=PAD, label_smoothing=0.1, mel_weight=10.0, sentence_avg=False, text_supervision=text)
    l64, c64 = R.forward(net, host, **kw)
    l32, _ = R.forward(net, host, dtype=torch.float32, **kw)
    lse = float(c64["lse_abs"].sum()) if text else 0.0
    for k in ("loss", "nll_loss", "mel_loss") + (("ctc_loss",) if text else ()):
        _gate(f"{name} valid_step {k}", log[k], l64[k], l32[k], abs(l64[k]) + (lse if k in ("loss", "ctc_loss") else 0.0))
    assert ("ctc_loss" in log) == text
    for k in ("n_correct", "total", "ntokens", "nsentences", "sample_size"):
        assert int(log[k]) == l64[k], k
    assert int(log["total"]) == sample["ntokens"]


@pytest.mark.parametrize("text", [False, True])
def test_valid_step_on_multi_target_avhubert(text):
    from lip2speech_unit_amd.conformer import ConformerConfig
    from lip2speech_unit_amd.hubert import AVHubertConfig
    from lip2speech_unit_amd.model_avhubert import MultiTargetAVHubertEncoderModel
    model = MultiTargetAVHubertEncoderModel.build_model(
        dtype=ops.F16, w2v_cfg=AVHubertConfig(encoder_layers=2),
        conformer_cfg=ConformerConfig(conformer_layers=2, text_supervision=text))
    model.load_state_dict(weights.synth_state_dict(weights.spec_of(model), seed=3))
    _check_valid_step(model.cuda().eval(), text, V_text=model.conformer.text_classes, name="multi_target_avhubert")


def test_valid_step_on_multi_target_raven():
    from lip2speech_unit_amd.conformer import ConformerConfig
    from lip2speech_unit_amd.model_raven import MultiTargetRAVENEncoderModel, RAVENConfig
    model = MultiTargetRAVENEncoderModel.build_model(dtype=ops.F16, encoder_cfg=RAVENConfig(encoder_num_blocks=2),
                                                     conformer_cfg=ConformerConfig(conformer_layers=2, text_supervision=False))
    model.load_state_dict(weights.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=81))
    _check_valid_step(model.cuda().eval(), False, name="multi_target_raven")


# ---- 7. CLI --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_validate_cli(tmp_path, capsys, dtype):
    from lip2speech_unit_amd import validate as v
    from tests._synth_dataset import make
    lab = make(str(tmp_path / "ds"), frames=(12, 9, 5))
    common = [f"override.data={lab}", f"override.label_dir={lab}", "synthetic_weights=true", "model.encoder_layers=2",
              "model.conformer_layers=2", f"dtype={dtype}"]
    out = str(tmp_path / "out")
    res = v.main(common + [f"common_eval.results_path={out}", "dataset.max_tokens=3600"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("valid | ")]
    assert len(line) == 1
    fields = [f.split()[0] for f in line[0].split(" | ")[1:]]
    assert fields == ["loss", "nll_loss", "ppl", "accuracy", "mel_loss"]
    saved = json.load(open(os.path.join(out, "valid-test.json")))
    assert saved["aggregate"] == res["aggregate"] and len(saved["clips"]) == 3
    assert [c["utt_id"] for c in saved["clips"]] == ["test/spk0/00000", "test/spk1/00001", "test/spk0/00002"]
    clips, tot = saved["clips"], saved["totals"]
    assert tot["loss"] == sum(c["loss"] for c in clips) and tot["nll_loss"] == sum(c["nll"] for c in clips)
    assert tot["mel_loss"] == sum(c["mel_loss"] for c in clips)
    assert tot["n_correct"] == sum(c["n_correct"] for c in clips) and tot["total"] == sum(c["n_tok"] for c in clips)
    assert [c["n_tok"] for c in clips] == [24, 18, 10] and [c["rows"] for c in clips] == [48, 36, 20]     # 2 / 4 x frames: clip-alone
    assert tot["ntokens"] == sum(c["ntokens"] for c in clips) == 25 + 20 + 11 and tot["sample_size"] == 3  # sentence_avg
    agg = saved["aggregate"]
    assert agg["loss"] == pytest.approx(tot["loss"] / 3 / np.log(2)) and agg["ppl"] == pytest.approx(2 ** agg["nll_loss"])
    assert agg["accuracy"] == pytest.approx(100.0 * tot["n_correct"] / tot["total"]) and np.isfinite(agg["loss"])
    # one clip per batch: every clip's partials are the same bytes
    out1 = str(tmp_path / "out1")
    res1 = v.main(common + [f"common_eval.results_path={out1}", "dataset.batch_size=1"])
    assert res1["clips"] == res["clips"]


def test_rows_past_2_31_elements():
    """A logits tensor of more than 2^31 elements (513 x 1024 rows of 4096): the last clip's rows start at element 2^31 exactly, so
    a 32-bit row offset anywhere would read the wrong rows.  Only the last clip has frames; the rest of the buffer is never read."""
    g = torch.Generator().manual_seed(23)
    B, T2, V, frames = 513, 1024, 4096, 24
    assert (B - 1) * T2 * V == 2 ** 31
    rows = torch.randn(2 * frames, V, generator=g) * 2
    big = torch.empty(B * T2, V, device="cuda")
    big[(B - 1) * T2:(B - 1) * T2 + 2 * frames] = rows.cuda()
    lens = torch.zeros(B, dtype=torch.int32)
    lens[-1] = frames
    target = torch.randint(4, V, (1, 2 * frames), generator=g)
    tgt = torch.full((B, 2 * frames), PAD, dtype=torch.int32)
    tgt[-1] = target[0]
    out = (torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, device="cuda", dtype=torch.int32),
           torch.empty(B, device="cuda", dtype=torch.int32))
    ops.unit_ce(big, tgt.cuda(), *out, B=B, T2=T2, V=V, lens=lens.cuda(), len_mul=2, pad_idx=PAD)
    c64 = R.unit_ce_per_clip(rows[None], target, [frames], PAD, torch.float64)
    c32 = R.unit_ce_per_clip(rows[None], target, [frames], PAD, torch.float32)
    _gate("unit nll past 2^31", out[0][-1:], c64["nll"], c32["nll"])
    _gate("unit smooth past 2^31", out[1][-1:], c64["smooth"], c32["smooth"])
    assert int(out[3][-1]) == 2 * frames and int(out[3][:-1].sum()) == 0 and float(out[0][:-1].abs().sum()) == 0.0
    labels = torch.tensor([9, 9, 300, 4000, 17], dtype=torch.int32)
    tl = torch.zeros(B, dtype=torch.int32)
    tl[-1] = len(labels)
    offs = torch.zeros(B, dtype=torch.int32)
    work = torch.empty(ops.ctc_loss_workspace_bytes(B, T2, len(labels)) // 4, device="cuda")
    nll = torch.empty(B, device="cuda")
    ops.ctc_loss(big, labels.cuda(), tl.cuda(), offs.cuda(), work, nll, B=B, L=T2, V=V, S_max=len(labels), lens=lens.cuda(), len_mul=2)
    n64, n32 = (_torch_ctc(rows[None], [labels], [frames], dt) for dt in (torch.float64, torch.float32))
    s_abs = torch.logsumexp(rows.double(), -1).abs().sum() + n64.abs()
    _gate("ctc past 2^31", nll[-1:], n64, n32, s_abs)
    assert float(nll[:-1].abs().sum()) == 0.0                    # clips without frames: 0
