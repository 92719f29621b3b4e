"""fp64 restatement of the unit decoders (csrc/decode.hip) for the glue matrix: greedy argmax and the exact n-best by dynamic programming.

Per step lp = log_softmax(x / temperature) over all V with the division done in fp32 exactly as the kernels do it, NaN -> -inf, ids 0..3
excluded.  Step scores do not depend on the history, so the best `n` sequences by additive score are found exactly by keeping the n best
prefixes per step with back pointers.  The forced EOS has lprob 0; the score is the sum divided by (L + 1)^lenpen.  oracle/decode.py is
the fp32 cross-check (tests/test_glue_matrix_cpu.py holds the two to each other)."""
import math

import torch

f64 = torch.float64
PAD, EOS = 1, 2


def step_lprobs(logits, temperature):
    """logits [L, V] fp32 -> (lp [L, V] fp64 with ids < 4 at -inf, x [L, V] fp64: the fp32 quotients, A [L, V]: the magnitudes behind lp)."""
    x = (logits.float() / torch.tensor(temperature, dtype=torch.float32)).to(f64)
    x = torch.where(torch.isnan(x), torch.full_like(x, -math.inf), x)
    mx = x.max(1, keepdim=True).values
    lse = (x - mx).exp().sum(1, keepdim=True).log()
    lp = x - mx - lse
    A = x.abs() + mx.abs() + lse.abs() + 1.0
    lp[:, :4] = -math.inf
    return lp, x, A


def greedy(logits, L, temperature, lenpen):
    """tokens [L + 1] (EOS last), lprobs [L + 1], A [L + 1], score, A of the score.  The argmax is taken on the fp32 quotients themselves
    (log_softmax is monotone), ties to the smaller id."""
    lp, x, A = step_lprobs(logits[:L], temperature)
    xu = x[:, 4:]
    V4 = xu.shape[1]
    best = xu.max(1, keepdim=True).values
    tok = torch.where(xu == best, torch.arange(V4).expand_as(xu), torch.full_like(xu, V4, dtype=torch.long)).min(1).values + 4
    rows = torch.arange(L)
    lps = torch.cat([lp[rows, tok], torch.zeros(1, dtype=f64)])
    As = torch.cat([A[rows, tok], torch.zeros(1, dtype=f64)])
    den = float(L + 1) ** lenpen
    return torch.cat([tok, torch.tensor([EOS])]), lps, As, lps.sum().item() / den, As.sum().item() / den


def nbest(logits, L, temperature, lenpen, n):
    """The n best sequences (fewer if there are fewer): tokens [n', L + 1], scores [n'] (normalised), best first."""
    if L == 0:
        return torch.full((1, 1), EOS, dtype=torch.long), torch.zeros(1, dtype=f64)
    lp = step_lprobs(logits[:L], temperature)[0]
    V = lp.shape[1]
    cum = torch.zeros(1, dtype=f64)
    bps, tks = [], []
    for s in range(L):
        cand = (cum[:, None] + lp[s][None, :]).reshape(-1)
        k = min(n, int((cand > -math.inf).sum()))
        cum, idx = torch.topk(cand, k)
        bps.append(idx // V)
        tks.append(idx % V)
    toks = torch.full((cum.numel(), L + 1), EOS, dtype=torch.long)
    cur = torch.arange(cum.numel())
    for s in range(L - 1, -1, -1):
        toks[:, s] = tks[s][cur]
        cur = bps[s][cur]
    return toks, cum / float(L + 1) ** lenpen


def score_of(lp, A, lenpen, tokens):
    """Positional scores, their A (the step's magnitudes plus the cumulative score's: they are differences of cumulative sums), the score and
    its A of a given unit sequence tokens [L]; lp, A: step_lprobs of the clip's first L steps."""
    L = tokens.numel()
    rows = torch.arange(L)
    pos = lp[rows, tokens]
    cum = pos.cumsum(0)
    Ap = A[rows, tokens] + cum.abs()
    den = float(L + 1) ** lenpen
    z = torch.zeros(1, dtype=f64)
    return torch.cat([pos, z]), torch.cat([Ap, z]), pos.sum().item() / den, Ap.sum().item() / den


def repeat_labels(x):
    """REPEAT_TEXT_LABELS as a python loop: a frame keeps the last non-zero label at or before it (label 0 until there is one)."""
    out, cur = [], x[0]
    for i, v in enumerate(x):
        if i and v != 0 and v != cur:
            cur = v
        out.append(cur)
    return out
