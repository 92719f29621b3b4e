"""float64 numpy restatements for Whisper on the device: the decoder-step kernels (csrc/whisper_decode.hip), the log-mel front end,
the encoder, the decoder and the greedy loop (weights in openai-whisper's layout), and the seeded case builders the tests share.
tests/test_whisper_cpu.py pins the model part to transformers.  Nothing here imports the package under test."""
import numpy as np


def softmax_attention(q, k, v):
    """q [H, 64], k / v [n, H, 64] (float64) -> [H, 64]: softmax over the n keys of q_h . k_jh, times v."""
    s = np.einsum("hc,jhc->hj", q, k)
    s = s - s.max(axis=1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=1, keepdims=True)
    return np.einsum("hj,jhc->hc", p, v)


def kv_attention(q, k_cache, v_cache, valid, k_new=None, v_new=None):
    """q [B, H, 64]; caches [B, T, H, 64]; valid: int [B]; with k_new / v_new [B, H, 64] the row valid[b] - 1 is taken from them.
    Returns (out [B, H, 64], k_cache', v_cache')."""
    B = q.shape[0]
    kc, vc = k_cache.copy(), v_cache.copy()
    out = np.zeros_like(q)
    for b in range(B):
        n = int(valid[b])
        if k_new is not None and n >= 1:
            kc[b, n - 1], vc[b, n - 1] = k_new[b], v_new[b]
        if n:
            out[b] = softmax_attention(q[b], kc[b, :n], vc[b, :n])
    return out, kc, vc


def masked_argmax(logits, forbid):
    """logits [B, V] float64, forbid bool [V] -> (ids [B] (first maximum of the allowed ids), log softmax of it over the allowed ids,
    margin [B] to the runner-up among the allowed ids (inf when only one is allowed))."""
    allowed = np.flatnonzero(~forbid)
    sub = logits[:, allowed]
    j = sub.argmax(axis=1)                      # numpy returns the first maximum
    ids = allowed[j]
    top = sub[np.arange(len(j)), j]
    lse = top + np.log(np.exp(sub - top[:, None]).sum(axis=1))
    if len(allowed) > 1:
        rest = sub.copy()
        rest[np.arange(len(j)), j] = -np.inf
        margin = top - rest.max(axis=1)
    else:
        margin = np.full(len(j), np.inf)
    return ids, top - lse, margin


def advance(token, logprob, tokens, sum_logprob, lengths, done, tok_emb, pos_emb, pos, eot):
    """One bookkeeping step on copies; returns the dict of new values (x_next is None when pos + 1 has no position row)."""
    V = tok_emb.shape[0]
    t = np.where(done, eot, token)
    t = np.where((t < 0) | (t >= V), eot, t)
    tokens = tokens.copy()
    if pos < tokens.shape[1]:
        tokens[:, pos] = t
    live = ~done
    sum_logprob = np.where(live, sum_logprob + logprob, sum_logprob)
    lengths = lengths + (live & (t != eot))
    done = done | (t == eot)
    x_next = tok_emb[t] + pos_emb[pos + 1] if pos + 1 < pos_emb.shape[0] else None
    return dict(token=t, tokens=tokens, sum_logprob=sum_logprob, lengths=lengths, done=done, x_next=x_next, pos=pos + 1,
                n_active=int((~done).sum()))


# ---- seeded cases ------------------------------------------------------------------------------------------------------------------

def attention_case(seed, B, H, T, round16):
    """Random 16-bit-representable q (scaled by 64^-0.5), caches and new rows.  Clip 1's keys carry a spike on the LAST row of every
    prefix length the tests use that is a multiple of 64 or one past it, so the running maximum of the online softmax jumps late."""
    rng = np.random.default_rng(seed)
    q = round16(rng.standard_normal((B, H, 64)) * 0.125)
    k = round16(rng.standard_normal((B, T, H, 64)))
    v = round16(rng.standard_normal((B, T, H, 64)))
    kn = round16(rng.standard_normal((B, H, 64)))
    vn = round16(rng.standard_normal((B, H, 64)))
    if B > 1:
        for j in (63, 64, 446, 447, T - 1):
            if 0 <= j < T:
                k[1, j] = round16(q[1] * (40.0 + j / 100.0))       # score ~ 40 |q|^2 ~ 40: far above the N(0, 1) scores of the rest
    return q, k, v, kn, vn


def vocab_case(seed, V, d, B, round16, plant_scale=0.05, sigma=0.05):
    """x [B, d], emb [V, d] (float32 arrays of 16-bit representable values), with per clip b: row top[b] = plant_scale * x_b (the decisive maximum), row
    second[b] = 0.8 of it (what wins once top[b] is suppressed), and dup[b] > top[b], an exact copy of row top[b] (a tie): in the
    next register of the same lane (b % 3 == 0), in another wave's rows of the tile (1) or in another tile (2)."""
    rng = np.random.default_rng(seed)
    x = round16(rng.standard_normal((B, d), dtype=np.float32))
    emb = round16(rng.standard_normal((V, d), dtype=np.float32) * np.float32(sigma))
    step = V // (B + 1)
    top = np.array([4 * ((3 + b * step) // 4) for b in range(B)])          # multiples of 4: register 0 of a lane
    off = np.array([(1, 17, 130)[b % 3] for b in range(B)])
    dup = top + off
    second = top + 2
    assert dup.max() < V and len(set(top) | set(dup) | set(second)) == 3 * B
    for b in range(B):
        emb[top[b]] = round16(x[b] * np.float32(plant_scale))
        emb[dup[b]] = emb[top[b]]
        emb[second[b]] = round16(x[b] * np.float32(plant_scale * 0.8))
    return x, emb, top, dup, second


# ---- the model: front end, encoder, decoder, greedy loop (float64; weights in OpenAI's layout) -----------------------------------

N_SAMPLES, N_FRAMES, N_FFT, HOP, N_MELS = 480000, 3000, 400, 160, 80


def _hz_to_mel(f):
    f = np.asarray(f, np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) * (27.0 / np.log(6.4)), 3.0 * f / 200.0)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), 200.0 * m / 3.0)


def mel_filters():
    """Slaney-scale, Slaney-normalised triangles: float64 [80, 201]."""
    freqs = np.linspace(0.0, 8000.0, N_FFT // 2 + 1)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(8000.0), N_MELS + 2))
    ramps = edges[:, None] - freqs[None, :]
    lower, upper = -ramps[:-2] / np.diff(edges)[:-1, None], ramps[2:] / np.diff(edges)[1:, None]
    return np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (edges[2:] - edges[:-2]))[:, None]


def power_frames(wav):
    """wav float [n <= 480000] -> the power spectrum float64 [3000, 201] of the zero-extended, reflect-padded clip."""
    x = np.zeros(N_SAMPLES, np.float64)
    x[: len(wav)] = wav
    x = np.pad(x, N_FFT // 2, mode="reflect")
    idx = HOP * np.arange(N_FRAMES)[:, None] + np.arange(N_FFT)[None, :]
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)
    return np.abs(np.fft.rfft(x[idx] * win, axis=1)) ** 2


def log_mel(wav, dtype=np.float64):
    """Whisper's input features [3000, 80].  dtype = float32 evaluates the band sums, the logarithm and the scaling in float32
    (on the float64 power spectrum rounded once): the yardstick for the device's fp32 values."""
    p = power_frames(wav).astype(dtype)
    mel = p @ mel_filters().astype(dtype).T
    x = np.log10(np.maximum(mel, dtype(1e-10)))
    x = np.maximum(x, x.max() - dtype(8.0))
    return (x + dtype(4.0)) / dtype(4.0)


def sinusoids(length, channels):
    inc = np.log(10000.0) / (channels // 2 - 1)
    t = np.arange(length)[:, None] * np.exp(-inc * np.arange(channels // 2))[None, :]
    return np.concatenate([np.sin(t), np.cos(t)], axis=1)


def _erf(x):
    try:
        from scipy.special import erf
        return erf(x)
    except ImportError:
        from math import erf
        return np.vectorize(erf, otypes=[np.float64])(x)


def _gelu(x):
    return 0.5 * x * (1.0 + _erf(x / np.sqrt(2.0)))


def _ln(x, sd, p):
    m = x.mean(axis=-1, keepdims=True)
    v = ((x - m) ** 2).mean(axis=-1, keepdims=True)
    return (x - m) / np.sqrt(v + 1e-5) * sd[p + ".weight"] + sd[p + ".bias"]


def _lin(x, sd, p):
    y = x @ sd[p + ".weight"].T
    return y + sd[p + ".bias"] if p + ".bias" in sd else y


def _heads(x, H):
    return x.reshape(x.shape[0], H, 64).transpose(1, 0, 2)          # [H, T, 64]


def _attend(q, k, v, H, causal):
    q, k, v = _heads(q, H), _heads(k, H), _heads(v, H)
    s = (q @ k.transpose(0, 2, 1)) * 0.125
    if causal:
        s = s + np.triu(np.full(s.shape[1:], -np.inf), 1)[None]
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    return (p @ v).transpose(1, 0, 2).reshape(q.shape[1], H * 64)


def _block(x, sd, p, H, xa=None, causal=False):
    h = _ln(x, sd, p + ".attn_ln")
    x = x + _lin(_attend(_lin(h, sd, p + ".attn.query"), _lin(h, sd, p + ".attn.key"), _lin(h, sd, p + ".attn.value"), H, causal),
                 sd, p + ".attn.out")
    if xa is not None:
        h = _ln(x, sd, p + ".cross_attn_ln")
        x = x + _lin(_attend(_lin(h, sd, p + ".cross_attn.query"), _lin(xa, sd, p + ".cross_attn.key"),
                             _lin(xa, sd, p + ".cross_attn.value"), H, False), sd, p + ".cross_attn.out")
    h = _ln(x, sd, p + ".mlp_ln")
    return x + _lin(_gelu(_lin(h, sd, p + ".mlp.0")), sd, p + ".mlp.2")


def _conv(x, w, b, stride):
    """x [T, Cin], w [Cout, Cin, 3], padding 1 -> [T / stride, Cout]."""
    xp = np.pad(x, ((1, 1), (0, 0)))
    T = x.shape[0]
    return sum(xp[k: k + T: stride] @ w[:, :, k].T for k in range(3)) + b


def encoder(sd, dims, feats):
    """feats [3000, 80] -> [1500, d]."""
    x = _gelu(_conv(feats, sd["encoder.conv1.weight"], sd["encoder.conv1.bias"], 1))
    x = _gelu(_conv(x, sd["encoder.conv2.weight"], sd["encoder.conv2.bias"], 2))
    x = x + sd["encoder.positional_embedding"]
    for i in range(dims["n_audio_layer"]):
        x = _block(x, sd, f"encoder.blocks.{i}", dims["n_audio_head"])
    return _ln(x, sd, "encoder.ln_post")


def decoder_logits(sd, dims, xa, tokens):
    """Teacher-forced: tokens int [n] -> logits float64 [n, V] (row i: the distribution of token i + 1)."""
    tokens = np.asarray(tokens)
    x = sd["decoder.token_embedding.weight"][tokens] + sd["decoder.positional_embedding"][: len(tokens)]
    for i in range(dims["n_text_layer"]):
        x = _block(x, sd, f"decoder.blocks.{i}", dims["n_text_head"], xa=xa, causal=True)
    return _ln(x, sd, "decoder.ln") @ sd["decoder.token_embedding.weight"].T


def greedy(sd, dims, xa, sot_sequence, eot, suppress, begin_suppress, max_new_tokens):
    """Greedy decoding at temperature 0.  Returns (ids of the sampled positions up to and without eot, per-step margin between the
    best and second-best allowed logit, sum of the chosen ids' log-probabilities incl. eot's, the step that produced eot or None)."""
    V = sd["decoder.token_embedding.weight"].shape[0]
    forbid = np.zeros(V, bool)
    forbid[list(suppress)] = True
    first = forbid.copy()
    first[list(begin_suppress)] = True
    toks, ids, margins, total, end = list(sot_sequence), [], [], 0.0, None
    for step in range(max_new_tokens):
        if len(toks) >= sd["decoder.positional_embedding"].shape[0]:
            break
        row = decoder_logits(sd, dims, xa, toks)[-1:]
        t, lp, m = masked_argmax(row, first if step == 0 else forbid)
        margins.append(float(m[0]))
        total += float(lp[0])
        if eot is not None and int(t[0]) == eot:
            end = step
            break
        ids.append(int(t[0]))
        toks.append(int(t[0]))
    return ids, margins, total, end


# ---- the seeded tiny model and clips ---------------------------------------------------------------------------------------------

TINY_DIMS = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=128, n_audio_head=2, n_audio_layer=2, n_vocab=333, n_text_ctx=64,
                 n_text_state=128, n_text_head=2, n_text_layer=2)
TINY_SOT = (330, 332)                          # the forced prefix of the tiny cases
TINY_SUPPRESS = (5, 17, 329, 330, 331, 332)
CLIP_SAMPLES = (32032, 64000, 48005)           # 2.002 s, 4 s, 3.0003 s


def tiny_state_dict(seed, dims=TINY_DIMS, std=0.15, final_gain=4.0):
    """Every matrix, bias and learned position N(0, std); LayerNorm gains 1 + N(0, std); the decoder's final gain times final_gain
    (a random Whisper at its default initialisation decodes one token for ever).  float64, OpenAI's names."""
    rng = np.random.default_rng(seed)
    d, dt, F = dims["n_audio_state"], dims["n_text_state"], 4 * dims["n_audio_state"]
    sd = {}

    def mat(name, *shape):
        sd[name] = rng.standard_normal(shape) * std

    def ln(name, n, gain=1.0):
        sd[name + ".weight"] = gain * (1.0 + rng.standard_normal(n) * std)
        mat(name + ".bias", n)

    def attn(p, n):
        for part in ("query", "key", "value", "out"):
            mat(f"{p}.{part}.weight", n, n)
            if part != "key":
                mat(f"{p}.{part}.bias", n)

    def block(p, n, cross):
        attn(p + ".attn", n), ln(p + ".attn_ln", n)
        if cross:
            attn(p + ".cross_attn", n), ln(p + ".cross_attn_ln", n)
        mat(p + ".mlp.0.weight", 4 * n, n), mat(p + ".mlp.0.bias", 4 * n), mat(p + ".mlp.2.weight", n, 4 * n), mat(p + ".mlp.2.bias", n)
        ln(p + ".mlp_ln", n)

    mat("encoder.conv1.weight", d, dims["n_mels"], 3), mat("encoder.conv1.bias", d)
    mat("encoder.conv2.weight", d, d, 3), mat("encoder.conv2.bias", d)
    sd["encoder.positional_embedding"] = sinusoids(dims["n_audio_ctx"], d)
    for i in range(dims["n_audio_layer"]):
        block(f"encoder.blocks.{i}", d, False)
    ln("encoder.ln_post", d)
    mat("decoder.token_embedding.weight", dims["n_vocab"], dt)
    mat("decoder.positional_embedding", dims["n_text_ctx"], dt)
    for i in range(dims["n_text_layer"]):
        block(f"decoder.blocks.{i}", dt, True)
    ln("decoder.ln", dt, gain=final_gain)
    return sd


def tiny_clips(seed=11):
    """Three int16 clips (FM tones plus noise) of CLIP_SAMPLES samples."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(CLIP_SAMPLES):
        t = np.arange(n) / 16000.0
        f0, dev, rate = 180.0 + 90.0 * i, 60.0 + 25.0 * i, 2.0 + 1.3 * i
        x = 0.35 * np.sin(2 * np.pi * f0 * t + dev / rate * np.sin(2 * np.pi * rate * t)) + 0.15 * np.sin(2 * np.pi * 3.1 * f0 * t)
        x = x * (0.6 + 0.4 * np.sin(2 * np.pi * (0.7 + 0.4 * i) * t)) + 0.03 * rng.standard_normal(n)
        out.append(np.round(x * 32767.0 * 0.8).astype(np.int16))
    return out


def round_state_dict(sd, round16):
    return {k: round16(v) for k, v in sd.items()}


# ---- the cases the tests share ----------------------------------------------------------------------------------------------------
# Seed search (tiny_state_dict seeds 0 .. 59, 10 greedy steps x 3 clips, float64): the three id sequences differ pairwise with >= 4
# distinct ids each for 21 seeds; of those only seed 26 keeps every step's margin >= 8 eps for fp16 (smallest margin 0.419 against
# eps = 0.0286, the largest logit error of this restatement with fp16-rounded weights and features).  For bf16 (eps = 0.279) no
# seed does, at 10 steps or fewer with >= 4 distinct ids; bf16 is checked at the steps whose margin reaches 8 eps (tests/
# test_whisper_cpu.py counts them).
TINY_SEED, TINY_STEPS = 26, 10
# id 328 is an ordinary id of the float64 decode: clip 0 emits it at step 4, clips 1 and 2 at step 6 and none at step 0 - as eot it
# ends the clips at different steps, all before the cap of 10
TINY_EOT = 328
TINY_BEGIN_SUPPRESS = (7, TINY_EOT)
_CASE = {}


def tiny_case():
    """The shared float64 case, computed once: weights, clips, features, encoder outputs, the free-running decode (no eot) and the
    decode with TINY_EOT."""
    if not _CASE:
        sd = tiny_state_dict(TINY_SEED)
        clips = tiny_clips()
        feats = [log_mel(c.astype(np.float64) / 32768.0) for c in clips]
        xa = [encoder(sd, TINY_DIMS, f) for f in feats]
        free = [greedy(sd, TINY_DIMS, x, TINY_SOT, None, TINY_SUPPRESS, TINY_BEGIN_SUPPRESS, TINY_STEPS) for x in xa]
        ended = [greedy(sd, TINY_DIMS, x, TINY_SOT, TINY_EOT, TINY_SUPPRESS, TINY_BEGIN_SUPPRESS, TINY_STEPS) for x in xa]
        _CASE.update(sd=sd, clips=clips, feats=feats, xa=xa, free=free, ended=ended)
    return _CASE


def quantised_logit_error(case, round16):
    """eps: the largest |logit| error of this restatement with weights and input features rounded by round16, teacher-forced on the
    float64 ids of the free decode; (eps over all steps, per-(clip, step) errors [3, steps])."""
    sd, sdq = case["sd"], round_state_dict(case["sd"], round16)
    P = len(TINY_SOT)
    err = []
    for c in range(len(case["clips"])):
        toks = list(TINY_SOT) + case["free"][c][0]
        lq = decoder_logits(sdq, TINY_DIMS, encoder(sdq, TINY_DIMS, round16(case["feats"][c])), toks[:-1])[P - 1:]
        l0 = decoder_logits(sd, TINY_DIMS, case["xa"][c], toks[:-1])[P - 1:]
        err.append(np.abs(lq - l0).max(axis=1))
    err = np.array(err)
    return float(err.max()), err


def log_mel_f32(wav):
    """The features evaluated in float32 throughout (frames times the windowed DFT table as a float32 product, powers, band sums,
    logarithm, clamp and scale): the yardstick for the device's fp32 values.  Returns float32 [3000, 80]."""
    x = np.zeros(N_SAMPLES, np.float64)
    x[: len(wav)] = wav
    x = np.pad(x, N_FFT // 2, mode="reflect").astype(np.float32)
    idx = HOP * np.arange(N_FRAMES)[:, None] + np.arange(N_FFT)[None, :]
    n, k = np.arange(N_FFT), np.arange(N_FFT // 2 + 1)
    ang = 2.0 * np.pi * ((n[:, None] * k[None, :]) % N_FFT) / N_FFT
    win = (0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT))[:, None]
    fr = x[idx]
    re, im = fr @ (win * np.cos(ang)).astype(np.float32), fr @ (-win * np.sin(ang)).astype(np.float32)
    mel = (re * re + im * im) @ mel_filters().astype(np.float32).T
    v = np.log10(np.maximum(mel, np.float32(1e-10)))
    v = np.maximum(v, v.max() - np.float32(8.0))
    return (v + np.float32(4.0)) / np.float32(4.0)
