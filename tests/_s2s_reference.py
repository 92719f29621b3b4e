"""Float64 numpy restatement of the AV-HuBERT seq2seq lip reader's decoder side: fairseq's
TransformerDecoderLayer / MultiheadAttention / SinusoidalPositionalEmbedding as avhubert/decoder.py composes them, the contracts of
l2s_beam_attention / l2s_beam_select / l2s_beam_advance, and the whole beam search of fairseq's sequence_generator.py with the
stated tie rule (equal scores: the smaller flat index slot * V + token first).  fairseq cannot be imported where the tests run, so
there is no golden file from it; tests/test_lipread_cpu.py pins this file against torch.nn.TransformerDecoderLayer, against its own
teacher-forced pass, against greedy decoding and against hand-computed table entries.

Token ids: 0 <s>, 1 <pad>, 2 </s> (eos, also the first input token), 3 <unk>."""
import math

import numpy as np

BOS, PAD, EOS, UNK = 0, 1, 2, 3
NEG = -np.inf


# ---- rounding to the 16-bit operand types ------------------------------------------------------------------------------------------
def round16(x, kind):
    """x (float64) rounded to fp16 / bf16 (round to nearest even) and back; kind None: unchanged."""
    x = np.asarray(x, dtype=np.float64)
    if kind is None:
        return x
    if kind == "fp16":
        return x.astype(np.float16).astype(np.float64)
    f = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    f = ((f + 0x7FFF + ((f >> 16) & 1)) >> 16) << 16
    return f.astype(np.uint32).view(np.float32).astype(np.float64)


# ---- positions ----------------------------------------------------------------------------------------------------------------------
def sinusoidal_table(n_rows, d, padding_idx=1):
    """fairseq's SinusoidalPositionalEmbedding.get_embedding: row[pos] = [sin(pos inv_k) | cos(pos inv_k)], k < d / 2,
    inv_k = exp(-k ln(10000) / (d / 2 - 1)); the padding row is zero.  Token index t of a history reads row t + padding_idx + 1."""
    half = d // 2
    inv = np.exp(-np.arange(half, dtype=np.float64) * (math.log(10000.0) / (half - 1)))
    ang = np.arange(n_rows, dtype=np.float64)[:, None] * inv[None, :]
    tab = np.concatenate([np.sin(ang), np.cos(ang)], axis=1)
    if d % 2:
        tab = np.concatenate([tab, np.zeros((n_rows, 1))], axis=1)
    tab[padding_idx] = 0.0
    return tab


def token_positions(n_tokens, d):
    """Rows of the table for token indices 0 .. n_tokens - 1 (table rows 2 ..)."""
    return sinusoidal_table(n_tokens + 2, d)[2:]


# ---- weights ------------------------------------------------------------------------------------------------------------------------
def tiny_state_dict(seed, d, heads, layers=2, V=36, d_enc=None, ffn=None, std=0.15, final_gain=6.0, share=True, wstd=None):
    """A decoder under fairseq's names (prefix `decoder.`): the embeddings N(0, std), every other matrix and bias N(0, wstd),
    LayerNorm gains 1 + N(0, wstd), the final LayerNorm's gain times final_gain so that the logits are peaked."""
    rng = np.random.default_rng(seed)
    d_enc = d_enc or d
    ffn = ffn or 2 * d
    wstd = std if wstd is None else wstd
    sd = {"decoder.embed_tokens.weight": rng.normal(0.0, std, size=(V, d))}
    g = lambda *s: rng.normal(0.0, wstd, size=s)
    sd["decoder.embed_tokens.weight"][PAD] = 0.0

    def ln(name, gain=1.0):
        sd[name + ".weight"] = (1.0 + g(d)) * gain
        sd[name + ".bias"] = g(d)
    for n in range(layers):
        p = f"decoder.layers.{n}."
        for a, kd in (("self_attn", d), ("encoder_attn", d_enc)):
            for m in "qkvo":
                name = p + a + "." + ("out" if m == "o" else m) + "_proj"
                sd[name + ".weight"] = g(d, kd if m in "kv" else d)
                sd[name + ".bias"] = g(d)
        ln(p + "self_attn_layer_norm"), ln(p + "encoder_attn_layer_norm"), ln(p + "final_layer_norm")
        sd[p + "fc1.weight"], sd[p + "fc1.bias"] = g(ffn, d), g(ffn)
        sd[p + "fc2.weight"], sd[p + "fc2.bias"] = g(d, ffn), g(d)
    ln("decoder.layer_norm", gain=final_gain)
    if not share:
        sd["decoder.embed_out"] = g(V, d)
    return sd


def tiny_encoder(seed, lens, T, d_enc, std=1.0):
    """Encoder rows [B, T, d_enc] N(0, std); rows at or past a clip's length are NaN (they must never be read)."""
    rng = np.random.default_rng(1000 + seed)
    enc = rng.normal(0.0, std, size=(len(lens), T, d_enc))
    for b, n in enumerate(lens):
        enc[b, n:] = np.nan
    return enc


# ---- the decoder --------------------------------------------------------------------------------------------------------------------
def layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def softmax(s):
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(-1, keepdims=True)


class Decoder:
    """The pre-LN (decoder_normalize_before) decoder.  kind: None = float64 throughout; "fp16" / "bf16" = weights and
    the activations the device keeps in 16 bits (LayerNorm outputs, q / k / v, attention outputs, the FFN's hidden row, the
    encoder rows) rounded to that type, everything else float64."""

    def __init__(self, sd, heads, kind=None, embed_scale=1.0, pos_table=None):
        self.kind, self.H, self.embed_scale = kind, heads, embed_scale
        self.sd = {k: (round16(v, kind) if v.ndim == 2 else np.asarray(v, dtype=np.float64)) for k, v in sd.items()}
        self.emb = self.sd["decoder.embed_tokens.weight"]
        self.out = self.sd.get("decoder.embed_out", self.emb)
        self.V, self.d = self.emb.shape
        self.n_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("decoder.layers."))
        self.pos_table = pos_table

    def r(self, x):
        return round16(x, self.kind)

    def lin(self, x, name):
        return x @ self.sd[name + ".weight"].T + self.sd[name + ".bias"]

    def ln(self, x, name):
        return layer_norm(x, self.sd[name + ".weight"], self.sd[name + ".bias"])

    def attend(self, q, k, v, mask=None):
        """q [n, d] (scaled), k / v [m, d] -> [n, d]; mask [n, m] additive."""
        n, d = q.shape
        hd = d // self.H
        out = np.empty_like(q)
        for h in range(self.H):
            sl = slice(h * hd, (h + 1) * hd)
            s = q[:, sl] @ k[:, sl].T
            if mask is not None:
                s = s + mask
            out[:, sl] = softmax(s) @ v[:, sl]
        return out

    def embed(self, tokens):
        n = len(tokens)
        pos = self.pos_table[:n] if self.pos_table is not None else token_positions(n, self.d)
        return self.embed_scale * self.emb[np.asarray(tokens)] + pos

    def layer(self, x, n, enc, cross_kv=None):
        """x [n, d] all positions of one history (causal), enc [m, d_enc] the clip's valid encoder rows."""
        p = f"decoder.layers.{n}."
        hd = self.d // self.H
        T = x.shape[0]
        causal = np.triu(np.full((T, T), NEG), 1)
        res = x
        h = self.r(self.ln(x, p + "self_attn_layer_norm"))
        q = self.r(self.lin(h, p + "self_attn.q_proj") * hd ** -0.5)
        k, v = self.r(self.lin(h, p + "self_attn.k_proj")), self.r(self.lin(h, p + "self_attn.v_proj"))
        x = res + self.lin(self.r(self.attend(q, k, v, causal)), p + "self_attn.out_proj")
        res = x
        h = self.r(self.ln(x, p + "encoder_attn_layer_norm"))
        q = self.r(self.lin(h, p + "encoder_attn.q_proj") * hd ** -0.5)
        ek, ev = cross_kv if cross_kv is not None else self.cross_kv(n, enc)
        x = res + self.lin(self.r(self.attend(q, ek, ev)), p + "encoder_attn.out_proj")
        res = x
        h = self.r(self.ln(x, p + "final_layer_norm"))
        f = self.r(np.maximum(self.lin(h, p + "fc1"), 0.0))
        x = res + self.lin(f, p + "fc2")
        return x

    def cross_kv(self, n, enc):
        p = f"decoder.layers.{n}.encoder_attn."
        e = self.r(enc)
        return self.r(self.lin(e, p + "k_proj")), self.r(self.lin(e, p + "v_proj"))

    def logits(self, tokens, enc, cross=None):
        """Teacher-forced: tokens [n] (index 0 = eos as bos) -> logits [n, V], row i the distribution of token i + 1."""
        x = self.embed(tokens)
        for n in range(self.n_layers):
            x = self.layer(x, n, enc, None if cross is None else cross[n])
        h = self.r(self.ln(x, "decoder.layer_norm"))
        return h @ self.out.T

    def all_cross(self, enc):
        return [self.cross_kv(n, enc) for n in range(self.n_layers)]


class Incremental:
    """One history decoded a token at a time against growing self caches (what the device does per slot)."""

    def __init__(self, dec, enc):
        self.dec, self.cross = dec, dec.all_cross(enc)
        self.k = [np.zeros((0, dec.d)) for _ in range(dec.n_layers)]
        self.v = [np.zeros((0, dec.d)) for _ in range(dec.n_layers)]
        self.n = 0

    def step(self, token):
        d = self.dec
        hd = d.d // d.H
        pos = d.pos_table[self.n] if d.pos_table is not None else token_positions(self.n + 1, d.d)[self.n]
        x = (d.embed_scale * d.emb[token] + pos)[None, :]
        for n in range(d.n_layers):
            p = f"decoder.layers.{n}."
            h = d.r(d.ln(x, p + "self_attn_layer_norm"))
            q = d.r(d.lin(h, p + "self_attn.q_proj") * hd ** -0.5)
            self.k[n] = np.concatenate([self.k[n], d.r(d.lin(h, p + "self_attn.k_proj"))], 0)
            self.v[n] = np.concatenate([self.v[n], d.r(d.lin(h, p + "self_attn.v_proj"))], 0)
            x = x + d.lin(d.r(d.attend(q, self.k[n], self.v[n])), p + "self_attn.out_proj")
            h = d.r(d.ln(x, p + "encoder_attn_layer_norm"))
            q = d.r(d.lin(h, p + "encoder_attn.q_proj") * hd ** -0.5)
            x = x + d.lin(d.r(d.attend(q, *self.cross[n])), p + "encoder_attn.out_proj")
            h = d.r(d.ln(x, p + "final_layer_norm"))
            x = x + d.lin(d.r(np.maximum(d.lin(h, p + "fc1"), 0.0)), p + "fc2")
        self.n += 1
        return (d.r(d.ln(x, "decoder.layer_norm")) @ d.out.T)[0]


# ---- kernel contracts ---------------------------------------------------------------------------------------------------------------
def beam_attention_self(q, kc, vc, k_new, v_new, anc, p, H, n_live=None, finished=None):
    """q / k_new / v_new [B, beam, W]; kc / vc [B, beam, L, W] (modified: row (b, i, p) <- new); anc [B, beam, L] -> out [B, beam, W]."""
    B, beam, W = q.shape
    hd = W // H
    out = np.zeros_like(q)
    for b in range(B):
        for i in range(beam):
            if (finished is not None and finished[b]) or (n_live is not None and i >= n_live[b]):
                continue
            kc[b, i, p], vc[b, i, p] = k_new[b, i], v_new[b, i]
            rows = [int(anc[b, i, t]) for t in range(p)]
            k = np.stack([kc[b, r, t] for t, r in enumerate(rows)] + [k_new[b, i]])
            v = np.stack([vc[b, r, t] for t, r in enumerate(rows)] + [v_new[b, i]])
            for h in range(H):
                sl = slice(h * hd, (h + 1) * hd)
                out[b, i, sl] = softmax(k[:, sl] @ q[b, i, sl]) @ v[:, sl]
    return out


def beam_attention_cross(q, kc, vc, enc_lens, H, n_live=None, finished=None):
    """q [B, beam, W]; kc / vc [B, T, W]; keys t < enc_lens[b]."""
    B, beam, W = q.shape
    hd = W // H
    out = np.zeros_like(q)
    for b in range(B):
        n = int(enc_lens[b])
        for i in range(beam):
            if (finished is not None and finished[b]) or (n_live is not None and i >= n_live[b]) or n <= 0:
                continue
            for h in range(H):
                sl = slice(h * hd, (h + 1) * hd)
                out[b, i, sl] = softmax(kc[b, :n, sl] @ q[b, i, sl]) @ vc[b, :n, sl]
    return out


def log_softmax_rows(y):
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.max(np.where(np.isnan(y), NEG, y), axis=-1, keepdims=True)
        lp = (y - m) - np.log(np.sum(np.exp(y - m), axis=-1, keepdims=True))
    return lp


def beam_select(logits, cum, step, max_len, beam, n_live=None, min_len=1, temperature=1.0, unk_penalty=0.0, extra=0):
    """One clip: logits [beam, V], cum [beam] -> (score, slot, token) of the 2 beam (+ extra) best, score descending, ties to the
    smaller flat index."""
    V = logits.shape[1]
    with np.errstate(invalid="ignore"):
        lp = log_softmax_rows(np.asarray(logits, dtype=np.float64) * (1.0 / temperature))
    lp[np.isnan(lp)] = NEG
    lp[:, PAD] = NEG
    lp[:, UNK] -= unk_penalty
    if step >= max_len:
        keep = lp[:, EOS].copy()
        lp[:] = NEG
        lp[:, EOS] = keep
    if step < min_len:
        lp[:, EOS] = NEG
    ns = 1 if step == 0 else (beam if n_live is None else n_live)
    s = (lp[:ns] + (0.0 if step == 0 else np.asarray(cum, dtype=np.float64)[:ns, None])).reshape(-1)
    order = np.lexsort((np.arange(s.size), -s))[:2 * beam + extra]          # score descending, then flat index ascending
    return s[order], order // V, order % V


class ClipState:
    """The device's per-clip search state (one half of the double buffers at a time)."""

    def __init__(self, beam, L):
        self.beam, self.L = beam, L
        self.tokens = np.full((beam, L), PAD, dtype=np.int64)
        self.tokens[:, 0] = EOS
        self.anc = np.zeros((beam, L), dtype=np.int64)
        self.anc[:, 0] = np.arange(beam)
        self.scores = np.zeros(beam)
        self.n_live, self.finished, self.step = beam, False, 0
        self.hyps = []                           # (tokens list, score) in finalisation order
        self.parents = np.zeros(beam, dtype=np.int64)
        self.out = None


def beam_advance(S, score, slot, token, max_len, lenpen=1.0, normalize=True):
    """One clip: books the candidates of S.step (see include/lip2speech_hip.h); returns the new slots' tokens."""
    if S.finished:
        return []
    beam, st = S.beam, S.step
    new = []
    for r in range(len(score)):
        if token[r] == EOS:
            if r < beam and score[r] > NEG and len(S.hyps) < beam:
                sc = score[r] / (st + 1) ** lenpen if normalize else score[r]
                S.hyps.append((list(S.tokens[slot[r], 1:st + 1]) + [EOS], sc))
        elif len(new) < beam:
            new.append(r)
    if len(S.hyps) >= beam or st >= max_len:
        S.finished, S.n_live = True, 0
        order = sorted(range(len(S.hyps)), key=lambda i: (-S.hyps[i][1], i))
        S.out = [S.hyps[i] for i in order]
        S.step += 1
        return []
    tok, anc, scores = S.tokens.copy(), S.anc.copy(), S.scores.copy()
    for j, r in enumerate(new):
        tok[j, :st + 1], anc[j, :st + 1] = S.tokens[slot[r], :st + 1], S.anc[slot[r], :st + 1]
        tok[j, st + 1], anc[j, st + 1] = token[r], j
        scores[j] = score[r]
        S.parents[j] = slot[r]
    S.tokens, S.anc, S.scores, S.n_live = tok, anc, scores, len(new)
    S.step += 1
    return [int(token[r]) for r in new]


# ---- the whole search ---------------------------------------------------------------------------------------------------------------
def clip_max_len(frames, max_len_a=1.0, max_len_b=0, max_target_positions=2048):
    return min(int(max_len_a * frames + max_len_b), max_target_positions - 1)


def search_clip(dec, enc, beam, max_len, min_len=1, lenpen=1.0, unk_penalty=0.0, temperature=1.0, normalize=True, follow=None):
    """Beam search of one clip (enc: its valid encoder rows).  Returns (hyps best first [(tokens, score)], trace): trace[step] =
    {"score", "slot", "token"} of the best 2 beam + 1 candidates.  follow = another run's trace: the decisions (which candidates, in
    which order) are taken from it and only the scores are this decoder's - how the 16-bit score error is measured."""
    L = max_len + 2
    S = ClipState(beam, L)
    cross = dec.all_cross(enc)
    trace = []
    while not S.finished:
        st = S.step
        ns = beam if st == 0 else S.n_live
        logits = np.full((beam, dec.V), 0.0)
        for i in range(ns):
            logits[i] = dec.logits(S.tokens[i, :st + 1], enc, cross)[-1]
        if follow is None:
            sc, sl, tk = beam_select(logits, S.scores, st, max_len, beam, n_live=S.n_live, min_len=min_len, temperature=temperature,
                                     unk_penalty=unk_penalty, extra=1)
        else:
            sl, tk = follow[st]["slot"], follow[st]["token"]
            lp = log_softmax_rows(logits * (1.0 / temperature))
            lp[:, UNK] -= unk_penalty
            sc = lp[sl, tk] + (0.0 if st == 0 else S.scores[sl])
            sc = np.where(np.isfinite(follow[st]["score"]), sc, NEG)
        trace.append({"score": sc, "slot": sl, "token": tk})
        K = 2 * beam
        beam_advance(S, sc[:K], sl[:K], tk[:K], max_len, lenpen=lenpen, normalize=normalize)
    return S.out, trace


def decisive(dec64, dec16, enc, beam, max_len, factor=4.0, **kw):
    """(is decisive, smallest gap, eps): eps = the largest |score error| of dec16 along dec64's search (candidate scores of every
    step and the final scores); decisive when every adjacent gap among the best 2 beam + 1 candidate scores of every step and among
    the final scores exceeds factor * eps."""
    hyps, trace = search_clip(dec64, enc, beam, max_len, **kw)
    hyps16, trace16 = search_clip(dec16, enc, beam, max_len, follow=trace, **kw)
    eps, gap = 0.0, np.inf
    for a, b in zip(trace, trace16):
        fin = np.isfinite(a["score"])
        if fin.any():
            eps = max(eps, float(np.max(np.abs(a["score"][fin] - b["score"][fin]))))
        s = a["score"][fin]
        if s.size > 1:
            gap = min(gap, float(np.min(s[:-1] - s[1:])))
    f64 = np.array([h[1] for h in hyps])
    f16 = np.array([h[1] for h in hyps16])
    if len(f64) == len(f16) and len(f64):
        eps = max(eps, float(np.max(np.abs(f64 - f16))))
    if len(f64) > 1:
        gap = min(gap, float(np.min(f64[:-1] - f64[1:])))
    return bool(gap > factor * eps), gap, eps, hyps


# ---- the seeded tiny cases shared by the CPU census and the GPU tests ------------------------------------------------------------------
TINY_V, TINY_LAYERS, TINY_T = 36, 2, 20
TINY_LENS = (1, 7, 20)
TINY_SHAPES = ((128, 2), (256, 2), (384, 2))     # (d, heads): head widths 64, 128, 192
TINY_BEAMS = (1, 3, 5)
TINY_GAIN, TINY_STD, TINY_WSTD = 6.0, 0.15, 0.03
TINY_MAX_LEN_A, TINY_MAX_LEN_B = 0.15, 2          # per-clip limits 2, 3 and 5 for 1, 7 and 20 frames: 3, 4 and 6 steps
# Seed search (seeds 0, 1, ... in order, float64 against the fp16-rounded restatement, all three clips): the first seed at which
# the case is decisive for fp16.  With these seeds every one of the 9 cases is decisive for fp16 (the census of
# tests/test_lipread_cpu.py asserts >= 75 %); for bf16 (eps about 10 x larger) only (256, 1) is, and bf16 is compared on the
# decisive cases only.
TINY_SEEDS = {(128, 1): 0, (128, 3): 1, (128, 5): 15, (256, 1): 1, (256, 3): 2, (256, 5): 22, (384, 1): 0, (384, 3): 6, (384, 5): 35}


def tiny_max_len(frames):
    return clip_max_len(frames, TINY_MAX_LEN_A, TINY_MAX_LEN_B)


def tiny_case(d, heads, beam):
    """(state dict, encoder rows [3, 20, d] with NaN padding, lens)."""
    seed = TINY_SEEDS[(d, beam)]
    return tiny_state_dict(seed, d, heads, TINY_LAYERS, TINY_V, std=TINY_STD, final_gain=TINY_GAIN, wstd=TINY_WSTD), \
        tiny_encoder(seed, TINY_LENS, TINY_T, d), TINY_LENS


_CENSUS = {}


def tiny_census(kind):
    """Per (d, heads, beam): (decisive for all three clips, [(decisive, gap, eps, hyps) per clip]) - the restatement alone, no
    device.  Computed once per kind and shared by the tests that need it."""
    if kind not in _CENSUS:
        out = {}
        for d, heads in TINY_SHAPES:
            for beam in TINY_BEAMS:
                sd, enc, lens = tiny_case(d, heads, beam)
                d64, d16 = Decoder(sd, heads), Decoder(sd, heads, kind=kind)
                clips = [decisive(d64, d16, enc[b, :n], beam, tiny_max_len(n)) for b, n in enumerate(lens)]
                out[(d, heads, beam)] = (all(c[0] for c in clips), clips)
        _CENSUS[kind] = out
    return _CENSUS[kind]


# One longer search, so that the ancestor table and the double buffers compose over 21 positions end to end: a clip of 20 encoder
# rows with limit 20 (max_len_a = 1) and min_len = 12, beam 3, d = 128.  Seeds 0 .. 599 were tried in order with the criterion
# above; 130 is the decisive one with the widest margin among the first ten found (smallest gap 0.110 against eps 0.0152).
TINY_LONG = {"d": 128, "heads": 2, "beam": 3, "seed": 130, "frames": 20, "max_len": 20, "min_len": 12}


def tiny_long_case():
    c = TINY_LONG
    sd = tiny_state_dict(c["seed"], c["d"], c["heads"], TINY_LAYERS, TINY_V, std=TINY_STD, final_gain=TINY_GAIN, wstd=TINY_WSTD)
    return sd, tiny_encoder(c["seed"], (c["frames"],), c["frames"], c["d"])


def tiny_long_census(kind):
    """(decisive, gap, eps, hyps) of the long case - computed once per kind."""
    key = ("long", kind)
    if key not in _CENSUS:
        c = TINY_LONG
        sd, enc = tiny_long_case()
        _CENSUS[key] = decisive(Decoder(sd, c["heads"]), Decoder(sd, c["heads"], kind=kind), enc[0], c["beam"], c["max_len"],
                                min_len=c["min_len"])
    return _CENSUS[key]
