"""Restatement of the `multi_target` criterion's forward (multi_target_lip2speech/criterion.py:52-146,182-201) in plain torch on
the CPU, in a chosen precision (float64 = the yardstick, float32 = "what the reference itself computes", whose distance from
float64 is the unit of the GPU gates).

What is pinned and what is recalled: the mel / spectral-convergence / CTC / logging part restates the reference's own program
text and is pinned by tests/golden/criterion.npz, which tools/make_criterion_golden.py wrote by RUNNING that text.  The base class
`LabelSmoothedCrossEntropyCriterion` is fairseq's and is not in the reference tree: `label_smoothed_nll_loss`, `compute_accuracy` and
the base-2 / ppl / accuracy-in-percent arithmetic of `reduce_metrics` are recalled from fairseq, not pinned (the tool that wrote
the golden file carries the same recollection as its stand-in, so the file cannot catch a misremembered base class).

`clip_alone` selects the product's row rule for the unit loss (a row also needs t < 2 * frames of its own clip); False is the
reference's (target != pad only).  The two agree whenever no clip has more labels than 2 * frames.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

N_MELS = 80


def unit_ce_per_clip(logits, target, lens, pad, dtype=torch.float64, clip_alone=True):
    """logits [B, T2, V], target int [B, Lt], lens int [B] video frames.  Returns dict of per-clip nll, smooth (dtype), n_correct,
    n_tok (int64) and the row mask [B, n]."""
    logits = torch.as_tensor(logits).to(dtype)
    target = torch.as_tensor(target).long()
    lens = torch.as_tensor(lens).long()
    n = min(logits.size(1), target.size(1))                                   # criterion.py:151-152
    lprobs = F.log_softmax(logits[:, :n], dim=-1)
    tgt = target[:, :n]
    mask = tgt.ne(pad)
    if clip_alone:
        mask = mask & (torch.arange(n)[None, :] < 2 * lens[:, None])
    safe = tgt.clamp(0, logits.size(-1) - 1)
    nll = (-lprobs.gather(-1, safe.unsqueeze(-1)).squeeze(-1)).masked_fill(~mask, 0.0)
    smooth = (-lprobs.sum(-1)).masked_fill(~mask, 0.0)
    correct = (lprobs.argmax(-1).eq(tgt) & mask)
    return {"nll": nll.sum(1), "smooth": smooth.sum(1), "n_correct": correct.sum(1), "n_tok": mask.sum(1), "mask": mask}


def mel_sums_per_clip(pred, targ, lens, dtype=torch.float64):
    """pred [B, Tp, 80], targ [B, Tt, 80] -> per-clip l1 = sum|p-t|, sq = sum (p-t)^2, tsq = sum t^2, rows (criterion.py:63-76)."""
    pred, targ = torch.as_tensor(pred).to(dtype), torch.as_tensor(targ).to(dtype)
    lens = torch.as_tensor(lens).long()
    crop = min(int(4 * lens.max()), pred.size(1), targ.size(1))               # :67
    p, t = pred[:, :crop], targ[:, :crop]
    m = (torch.arange(crop)[None, :] < 4 * lens[:, None])
    d = (p - t) * m[..., None]
    return {"l1": d.abs().sum((1, 2)), "sq": (d * d).sum((1, 2)), "tsq": ((t * m[..., None]) ** 2).sum((1, 2)), "rows": m.sum(1)}


def mel_loss_per_clip(sums, sentence_avg):
    """criterion.py:78-87 + :197-201 from the per-clip sums: masked L1 (mean over the 80 bins) + spectral convergence."""
    rows = sums["rows"].to(sums["l1"].dtype)
    l1 = sums["l1"] / N_MELS
    sc = sums["sq"].sqrt() / sums["tsq"].sqrt()
    return l1 / rows + sc if sentence_avg else l1 + sc * rows


def ctc_alpha_nll(logp, labels, blank=0):
    """-log p(labels | frames) by the alpha recursion in float64 numpy (Graves 2006), independent of torch's ctc_loss.
    logp [T, V] log-probabilities of one clip's own frames."""
    logp = np.asarray(logp, np.float64)
    T, S = logp.shape[0], len(labels)
    ext = [blank]
    for c in labels:
        ext += [int(c), blank]
    E = len(ext)
    if T == 0:
        return math.inf
    a = np.full(E, -np.inf)
    a[0] = logp[0, blank]
    if E > 1:
        a[1] = logp[0, ext[1]]
    skip = np.array([s >= 2 and ext[s] != blank and ext[s] != ext[s - 2] for s in range(E)])
    for t in range(1, T):
        b = np.full(E, -np.inf)
        b[1:] = a[:-1]
        c = np.full(E, -np.inf)
        c[2:] = np.where(skip[2:], a[:-2], -np.inf)
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.maximum(np.maximum(a, b), c)
            s = np.exp(a - m) + np.exp(b - m) + np.exp(c - m)
            new = np.where(np.isneginf(m), -np.inf, m + np.log(s))
        a = new + logp[t, ext]
    tail = a[-1] if E == 1 else np.logaddexp(a[-1], a[-2])
    return float(-tail)


def ctc_per_clip(text_logits, labels, label_lens, lens, dtype=torch.float64, blank=0):
    """text_logits [B, L, V]; labels 1-D concatenated; per-clip CTCLoss(blank, zero_infinity=True) (criterion.py:45,103-110) and
    sum_t |logsumexp_t| over the clip's own frames (the gate's size of what the loss accumulates)."""
    x = torch.as_tensor(text_logits).to(dtype)
    lp = F.log_softmax(x, dim=2).transpose(0, 1)                               # T x B x C
    il = (2 * torch.as_tensor(lens).long()).clamp(max=x.size(1))               # :107
    tl = torch.as_tensor(label_lens).long()
    nll = F.ctc_loss(lp, torch.as_tensor(labels).long(), il, tl, blank=blank, reduction="none", zero_infinity=True)
    lse = torch.logsumexp(x.double(), dim=2).abs()
    s_abs = torch.stack([lse[b, : int(il[b])].sum() for b in range(x.size(0))])
    return {"nll": nll, "lse_abs": s_abs}


def forward(net_output, sample, *, pad, label_smoothing, mel_weight, sentence_avg, text_supervision, report_accuracy=True,
            dtype=torch.float64, clip_alone=True):
    """criterion.py:52-146: returns (logging_output as python floats / ints, per-clip dict).  net_output: encoder_out [B, T2, V],
    encoder_out_mel [B, Tm, 80], encoder_out_text [L, B, Vt] (T x B x C, as the models give it); sample: target, input_lengths, mel,
    ntokens, text_labels, text_labels_lengths."""
    lens = torch.as_tensor(sample["input_lengths"]).long()
    ce = unit_ce_per_clip(net_output["encoder_out"], sample["target"], lens, pad, dtype, clip_alone)
    V = torch.as_tensor(net_output["encoder_out"]).size(-1)
    eps_i = label_smoothing / (V - 1)
    ce_loss = (1.0 - label_smoothing - eps_i) * ce["nll"] + eps_i * ce["smooth"]
    sums = mel_sums_per_clip(net_output["encoder_out_mel"], sample["mel"], lens, dtype)
    mel = mel_loss_per_clip(sums, sentence_avg)
    loss = ce_loss + mel_weight * mel
    B = len(lens)
    clip = {"nll": ce["nll"], "smooth": ce["smooth"], "n_correct": ce["n_correct"], "n_tok": ce["n_tok"], "mel_loss": mel,
            "l1": sums["l1"], "sq": sums["sq"], "tsq": sums["tsq"], "rows": sums["rows"]}
    sample_size = B if sentence_avg else int(sample["ntokens"])
    log = {"nll_loss": float(ce["nll"].sum()), "mel_loss": float(mel.sum()), "ntokens": int(sample["ntokens"]), "nsentences": B,
           "sample_size": sample_size}
    if text_supervision:
        text = torch.as_tensor(net_output["encoder_out_text"]).transpose(0, 1)
        ctc = ctc_per_clip(text, sample["text_labels"], sample["text_labels_lengths"], lens, dtype)
        loss = loss + ctc["nll"]
        log["ctc_loss"] = float(ctc["nll"].sum())
        clip["ctc_loss"], clip["lse_abs"] = ctc["nll"], ctc["lse_abs"]
    clip["loss"] = loss
    log["loss"] = float(loss.sum())
    if report_accuracy:
        log["n_correct"], log["total"] = int(ce["n_correct"].sum()), int(ce["n_tok"].sum())
    return log, clip


def reduce_metrics(logs):
    """fairseq's LabelSmoothedCrossEntropyCriterion.reduce_metrics (recalled) + criterion.py:163-179."""
    tot = lambda k: sum(float(l.get(k, 0)) for l in logs)       # noqa: E731
    ss, nt = tot("sample_size"), tot("ntokens")
    out = {"loss": tot("loss") / ss / math.log(2), "nll_loss": tot("nll_loss") / nt / math.log(2)}
    out["ppl"] = 2 ** out["nll_loss"]
    if tot("total") > 0:
        out["accuracy"] = tot("n_correct") * 100.0 / tot("total")
    if logs[0].get("mel_loss") is not None:
        out["mel_loss"] = tot("mel_loss") / ss
    if "ctc_loss" in logs[0]:
        out["ctc_loss"] = tot("ctc_loss") / ss
    return out


# ---- seeded cases (shared by tools/make_criterion_golden.py and the tests: the inputs are STORED in the golden file, this
# generator is only how they were drawn) ---------------------------------------------------------------------------------
def draw_case(seed, frames, label_counts, mel_lens, text_labels, V=204, Vt=256, pad=1, gap=1e-3):
    """frames: video frames per clip; label_counts: unit labels per clip (<= 2*frames keeps both row rules equal); mel_lens: target
    mel rows per clip; text_labels: list of label lists (ids in 1..Vt-1).  Logits are drawn so that every row's top-two gap is
    >= `gap` (the arg-max is well defined in any precision)."""
    g = torch.Generator().manual_seed(seed)
    B, T = len(frames), max(frames)
    logits = (torch.randn(B, 2 * T, V, generator=g) * 2.0).float()
    top = logits.topk(2, -1)
    bump = (top.values[..., 0] - top.values[..., 1]) < 4 * gap
    logits.scatter_add_(-1, top.indices[..., :1], (bump.float() * 16 * gap).unsqueeze(-1))
    Lt = max(label_counts)
    target = torch.full((B, Lt), pad, dtype=torch.long)
    for b, n in enumerate(label_counts):
        lab = torch.randint(4, V, (n,), generator=g)
        hit = torch.rand(n, generator=g) < 0.5                      # half the labels are the arg-max: accuracy is not trivially 0
        am = logits[b, :n].argmax(-1)
        target[b, :n] = torch.where(hit & (am >= 4), am, lab)
    mel_pred = torch.randn(B, 4 * T, N_MELS, generator=g).float()
    Tm = max(mel_lens)
    mel = torch.zeros(B, Tm, N_MELS)
    for b, n in enumerate(mel_lens):
        mel[b, :n] = torch.randn(n, N_MELS, generator=g) - 4.0
    text = torch.randn(2 * T, B, Vt, generator=g).float()
    pm = torch.arange(T)[None, :] >= torch.tensor(frames)[:, None]
    return {"encoder_out": logits, "encoder_out_mel": mel_pred, "encoder_out_text": text, "padding_mask": pm,
            "target": target, "ntokens": int(sum(label_counts)), "mel": mel,
            "input_lengths": torch.tensor(frames, dtype=torch.int32),
            "text_labels": torch.tensor([c for t in text_labels for c in t], dtype=torch.int32),
            "text_labels_lengths": torch.tensor([len(t) for t in text_labels], dtype=torch.int32)}


def top2_gap(logits, mask):
    """Smallest top-two gap over the counted rows."""
    top = torch.as_tensor(logits).double().topk(2, -1).values
    gaps = (top[..., 0] - top[..., 1])[:, : mask.size(1)][mask]
    return float(gaps.min()) if gaps.numel() else math.inf
