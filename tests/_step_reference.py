"""Generic float64 / exact restatements of the autoregressive decoding kernels' contracts (csrc/whisper_decode.hip, csrc/s2s_decode.hip) for
the step matrix (tests/_step_cases.py, tools/check_step_kernels.py): the same operations as tests/_whisper_reference.py and
tests/_s2s_reference.py state them, widened to what the entries document outside the callers' habits - a device position at or past the
cache, a negative one, ancestor entries outside the beam, live counts outside [0, beam], valid lengths outside [0, T], pad / unk rules
switched off, the no-room rule of l2s_beam_advance.  tests/test_step_matrix_cpu.py pins every function here to those two modules to 1e-12
(exactly where the operation is exact) on inputs inside their contracts.  numpy only."""
import numpy as np

NEG = -np.inf
U32 = 2.0 ** -24


def round16(x, dt):
    """x (float64) rounded to f16 / bf16 (round to nearest even) and back"""
    x = np.asarray(x, dtype=np.float64)
    if dt == "f16":
        return x.astype(np.float16).astype(np.float64)
    f = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    f = ((f + 0x7FFF + ((f >> 16) & 1)) >> 16) << 16
    return f.astype(np.uint32).view(np.float32).astype(np.float64)


def _softmax_rows(k, q, v):
    """k / v [n, hd], q [hd] -> softmax(k q) v"""
    s = k @ q
    s = s - s.max()
    e = np.exp(s)
    return (e / e.sum()) @ v


# ---- l2s_kv_attention ---------------------------------------------------------------------------------------------------------------------------
def kv_attention(q, kc, vc, H, pos=None, n_valid=0, k_new=None, v_new=None):
    """q [B, W]; kc / vc [B, T, W]; pos: int [B] (the device position of every clip) or None (n_valid rows); k_new / v_new [B, W] or None.
    valid = clamp(pos + 1 or n_valid, 0, T); the new row is stored at row pos, and read from there, only when 0 <= pos < T.
    Returns (out [B, W], kc', vc', read [B, T] bool: the cache rows the clip reads)."""
    B, T, W = kc.shape
    hd = W // H
    kc, vc = kc.copy(), vc.copy()
    out = np.zeros((B, W))
    read = np.zeros((B, T), bool)
    for b in range(B):
        p = -1 if pos is None else int(pos[b])
        valid = min(max(n_valid if pos is None else p + 1, 0), T)
        if k_new is not None and 0 <= p < T:
            kc[b, p], vc[b, p] = k_new[b], v_new[b]
        read[b, :valid] = True
        if k_new is not None and 0 <= p < T:
            read[b, p] = False                      # taken from the new rows themselves
        if valid:
            for h in range(H):
                sl = slice(h * hd, (h + 1) * hd)
                out[b, sl] = _softmax_rows(kc[b, :valid, sl], q[b, sl], vc[b, :valid, sl])
    return out, kc, vc, read


# ---- l2s_beam_attention -------------------------------------------------------------------------------------------------------------------------
def beam_dead(b, i, n_live, finished):
    return bool((finished is not None and finished[b]) or (n_live is not None and i >= n_live[b]))


def beam_attention_self(q, kc, vc, k_new, v_new, anc, p, H, n_live=None, finished=None):
    """q / k_new / v_new [B, beam, W]; kc / vc [B, beam, T, W]; anc [2, B, beam, T] (the half p & 1 is current; entries are clamped to
    [0, beam - 1]).  p < 0 or p >= T: every slot is dead.  Returns (out, kc', vc')."""
    B, beam, T, W = kc.shape
    hd = W // H
    kc, vc = kc.copy(), vc.copy()
    out = np.zeros((B, beam, W))
    if p < 0 or p >= T:
        return out, kc, vc
    cur = np.clip(np.asarray(anc)[p & 1], 0, beam - 1)
    k0, v0 = kc.copy(), vc.copy()                   # rows t < p are not written by this launch
    for b in range(B):
        for i in range(beam):
            if beam_dead(b, i, n_live, finished):
                continue
            kc[b, i, p], vc[b, i, p] = k_new[b, i], v_new[b, i]
            rows = [int(cur[b, i, t]) for t in range(p)]
            k = np.stack([k0[b, r, t] for t, r in enumerate(rows)] + [k_new[b, i]])
            v = np.stack([v0[b, r, t] for t, r in enumerate(rows)] + [v_new[b, i]])
            for h in range(H):
                sl = slice(h * hd, (h + 1) * hd)
                out[b, i, sl] = _softmax_rows(k[:, sl], q[b, i, sl], v[:, sl])
    return out, kc, vc


def beam_attention_cross(q, kc, vc, enc_lens, H, n_live=None, finished=None):
    """q [B, beam, W]; kc / vc [B, T, W]; keys t < clamp(enc_lens[b], 0, T)"""
    B, beam, W = q.shape
    T = kc.shape[1]
    hd = W // H
    out = np.zeros((B, beam, W))
    for b in range(B):
        n = min(max(int(enc_lens[b]), 0), T)
        for i in range(beam):
            if beam_dead(b, i, n_live, finished) or n == 0:
                continue
            for h in range(H):
                sl = slice(h * hd, (h + 1) * hd)
                out[b, i, sl] = _softmax_rows(kc[b, :n, sl], q[b, i, sl], vc[b, :n, sl])
    return out


# ---- l2s_vocab_argmax ---------------------------------------------------------------------------------------------------------------------------
def vocab_logits(x, emb):
    """float64 logits [B, V]"""
    x = np.asarray(x, np.float64)
    return np.concatenate([x @ np.asarray(emb[i:i + 8192], np.float64).T for i in range(0, emb.shape[0], 8192)], axis=1)


def vocab_logits_f32(x, emb):
    """two fp32 evaluations on the CPU: one BLAS product, and the chain the kernel runs (products ascending in k, 32 at a time)"""
    x32, e32 = np.asarray(x, np.float32), np.asarray(emb, np.float32)
    blas = x32 @ e32.T
    chain = np.zeros_like(blas)
    for k0 in range(0, x32.shape[1], 32):
        chain += x32[:, k0:k0 + 32] @ e32[:, k0:k0 + 32].T
    return blas, chain


def masked_argmax(logits, forbid):
    """(ids [B] first maximum among the allowed ids, -1 when none is allowed; log softmax of it over the allowed ids, -inf when none)"""
    B = logits.shape[0]
    allowed = np.flatnonzero(~forbid)
    if allowed.size == 0:
        return np.full(B, -1), np.full(B, NEG)
    sub = logits[:, allowed]
    j = sub.argmax(axis=1)
    top = sub[np.arange(B), j]
    return allowed[j], -np.log(np.exp(sub - top[:, None]).sum(axis=1))


# ---- l2s_whisper_advance ------------------------------------------------------------------------------------------------------------------------
def whisper_advance(token, logprob, tokens, sum_logprob, lengths, done, tok_emb, pos_emb, pos, eot, x_next):
    """Everything on copies, exact (fp32 where the kernel is fp32).  tokens [B, ld_tok]: column pos only when 0 <= pos < ld_tok; x_next
    [B, d] fp32: rewritten only when 0 <= pos + 1 < n_ctx; pos always advances."""
    V = tok_emb.shape[0]
    done = np.asarray(done, bool)
    t = np.where(done, eot, token)
    t = np.where((t < 0) | (t >= V), eot, t)
    tokens = tokens.copy()
    if 0 <= pos < tokens.shape[1]:
        tokens[:, pos] = t
    live = ~done
    slp = np.where(live, (sum_logprob.astype(np.float32) + logprob.astype(np.float32)).astype(np.float32), sum_logprob.astype(np.float32))
    lengths = lengths + (live & (t != eot))
    done2 = done | (t == eot)
    x_next = x_next.copy()
    if 0 <= pos + 1 < pos_emb.shape[0]:
        x_next[:] = tok_emb[t].astype(np.float32) + pos_emb[pos + 1].astype(np.float32)
    return dict(token=t, tokens=tokens, sum_logprob=slp, lengths=lengths, done=done2, x_next=x_next, pos=pos + 1, n_active=int((~done2).sum()))


# ---- l2s_beam_select ----------------------------------------------------------------------------------------------------------------------------
def log_softmax_rows(y):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.max(np.where(np.isnan(y), NEG, y), axis=-1, keepdims=True)
        return (y - m) - np.log(np.sum(np.exp(y - m), axis=-1, keepdims=True))


def beam_select(logits, cum, step, max_len, beam, n_live=None, min_len=1, temperature=1.0, unk_penalty=0.0, pad=1, unk=3, eos=2, extra=0):
    """One clip: logits [beam, V], cum [beam] -> (score, slot, token) of the 2 beam + extra best, score descending, ties (the -inf ones
    too) to the smaller flat index.  step <= 0: slot 0 alone, cum ignored; n_live is clamped to [1, beam]; pad / unk = -1: no rule."""
    V = logits.shape[1]
    with np.errstate(invalid="ignore"):
        lp = log_softmax_rows(np.asarray(logits, dtype=np.float64) * (1.0 / temperature))
    lp[np.isnan(lp)] = NEG
    if 0 <= pad < V:
        lp[:, pad] = NEG
    if 0 <= unk < V:
        lp[:, unk] -= unk_penalty
    if step >= max_len:
        keep = lp[:, eos].copy()
        lp[:] = NEG
        lp[:, eos] = keep
    if step < min_len:
        lp[:, eos] = NEG
    ns = 1 if step <= 0 else min(max(beam if n_live is None else int(n_live), 1), beam)
    s = (lp[:ns] + (0.0 if step <= 0 else np.asarray(cum, dtype=np.float64)[:ns, None])).reshape(-1)
    order = np.lexsort((np.arange(s.size), -s))[:2 * beam + extra]
    return s[order], order // V, order % V


def select_tol(V, s):
    """tests/test_lipread_kernels_gpu.py select_tol: fp32 against float64 for a compared candidate of score s"""
    return (V / 64 + 8 + 2 * 10) * U32 + 8 * U32 * (np.abs(s) + 10.0)


# ---- l2s_beam_advance ---------------------------------------------------------------------------------------------------------------------------
def advance_state(B, beam, L, d, pre_finished=None, pad=1, eos=2):
    """the device tables of a search before its first step, as numpy arrays of the device types (x: NaN = never written)"""
    S = dict(tokens=np.full((2, B, beam, L), pad, np.int32), anc=np.zeros((2, B, beam, L), np.int16), scores=np.zeros((2, B, beam), np.float32),
             n_live=np.full(B, beam, np.int32), finished=np.zeros(B, np.uint8), parents=np.zeros((B, beam), np.int32),
             hyp_tokens=np.full((B, beam, L), pad, np.int32), hyp_len=np.zeros((B, beam), np.int32), hyp_score=np.zeros((B, beam), np.float32),
             nhyp=np.zeros(B, np.int32), out_tokens=np.full((B, beam, L), pad, np.int32), out_len=np.zeros((B, beam), np.int32),
             out_score=np.full((B, beam), NEG, np.float32), x=np.full((B * beam, d), np.nan, np.float32), step=np.zeros(1, np.int32),
             n_active=np.zeros(1, np.int32))
    S["tokens"][:, :, :, 0] = eos
    S["anc"][:, :, :, 0] = np.arange(beam, dtype=np.int16)[None, None, :]
    if pre_finished is not None:
        S["finished"][:] = pre_finished
    return S


def beam_advance(S, cs, cl, ct, max_len, emb, pos_table, embed_scale, V, eos=2, pad=1, lenpen=1.0, normalize=True):
    """Books one step's candidates cs / cl / ct [B, 2 beam] into the tables S (in place), exactly as l2s_beam_advance documents it: a
    finished clip is inert; a clip with step < 0 or step + 1 >= L keeps every byte (no room for another token); cand_slot is clamped
    to [0, beam - 1] and cand_token to [0, V - 1] where they index; step advances and n_active counts the unfinished clips always.
    Every number is exact: hyp scores are one fp32 division, x one fp32 fma."""
    _, B, beam, L = S["tokens"].shape
    K = 2 * beam
    st = int(S["step"][0])
    cur, nxt = st & 1, (st & 1) ^ 1
    for b in range(B):
        if S["finished"][b] or st < 0 or st + 1 >= L:
            continue
        nh = min(max(int(S["nhyp"][b]), 0), beam)
        hyp = [np.float32(S["hyp_score"][b, i]) for i in range(nh)] + [np.float32(0)] * (beam - nh)
        denom = np.float32(np.float32(st + 1) ** np.float32(lenpen)) if normalize else np.float32(1.0)
        fin_r, fin_dst, new_r = [], [], []
        for r in range(K):
            if ct[b, r] == eos:
                if r < beam and cs[b, r] > NEG and nh < beam:
                    fin_r.append(r)
                    fin_dst.append(nh)
                    hyp[nh] = np.float32(np.float32(cs[b, r]) / denom)
                    nh += 1
            elif len(new_r) < beam:
                new_r.append(r)
        fin = nh >= beam or st >= max_len[b]
        tok_cur, anc_cur = S["tokens"][cur, b].copy(), S["anc"][cur, b].copy()
        for r, dst in zip(fin_r, fin_dst):
            parent = min(max(int(cl[b, r]), 0), beam - 1)
            row = np.full(L, pad, np.int32)
            row[:st] = tok_cur[parent, 1:st + 1]
            row[st] = eos
            S["hyp_tokens"][b, dst] = row
            S["hyp_len"][b, dst] = st + 1
            S["hyp_score"][b, dst] = hyp[dst]
        if not fin:
            for j, r in enumerate(new_r):
                parent = min(max(int(cl[b, r]), 0), beam - 1)
                S["tokens"][nxt, b, j, :st + 1] = tok_cur[parent, :st + 1]
                S["anc"][nxt, b, j, :st + 1] = anc_cur[parent, :st + 1]
                S["tokens"][nxt, b, j, st + 1] = ct[b, r]
                S["anc"][nxt, b, j, st + 1] = j
                S["scores"][nxt, b, j] = cs[b, r]
                S["parents"][b, j] = parent
                tk = min(max(int(ct[b, r]), 0), V - 1)
                # fmaf(scale, emb, pos): the product and the sum are exact in float64 for these operands, rounded once
                S["x"][b * beam + j] = (np.float64(np.float32(embed_scale)) * emb[tk].astype(np.float64) + pos_table[st + 1].astype(np.float64)).astype(np.float32)
        else:
            order = sorted(range(nh), key=lambda i: (-float(hyp[i]), i))
            nold = nh - len(fin_r)
            for rank, i in enumerate(order):
                S["out_tokens"][b, rank] = S["hyp_tokens"][b, i]
                S["out_len"][b, rank] = S["hyp_len"][b, i] if i < nold else st + 1
                S["out_score"][b, rank] = hyp[i]
        S["nhyp"][b] = nh
        S["n_live"][b] = 0 if fin else len(new_r)
        if fin:
            S["finished"][b] = 1
    S["step"][0] = st + 1
    S["n_active"][0] = int((S["finished"] == 0).sum())
    return S
