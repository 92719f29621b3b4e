"""The three decoder-step kernels of csrc/whisper_decode.hip on the device, each against float64 (tests/_whisper_reference.py):
l2s_kv_attention, l2s_vocab_argmax, l2s_whisper_advance.

Bounds.  Every compared quantity has two: 8 x the largest error measured on an MI355X over the cases of this file (MEASURED below,
the factor of tests/test_stoi_gpu.py), and an independent ceiling computed on the CPU that no measurement can loosen: 4 x the error
of the float64 result rounded once to the 16-bit output type (attention), 4 x the worst float32 CPU evaluation (fp32 logits and
log-probabilities; never below one float32 ulp at the value's scale).  The smaller of the two holds.  Every test prints its figure
as `MEASURE <key> <value>` before it asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import ops  # noqa: E402
from tests import _whisper_reference as R  # noqa: E402

DTYPES = [ops.F16, ops.BF16]
DNAME = {ops.F16: "f16", ops.BF16: "bf16"}
# largest |device - float64| seen on an MI355X, per quantity (MEASURE lines of this file)
MEASURED = {
    "attn_f16": 9.66e-4, "attn_bf16": 7.80e-3,          # half an ulp of the 16-bit output at |out| in [2, 4): the final rounding
    "logit_f16": 2.87e-5, "logit_bf16": 3.58e-5,        # at d = 1280 (|logit| up to 64); 5.5e-7 / 6.8e-7 at d = 128
    "logprob_f16": 5.87e-7, "logprob_bf16": 3.16e-7,
}


def _bound(key, value, ceiling):
    print(f"MEASURE {key} {value:.3e} ceiling {ceiling:.3e}")
    return min(8.0 * MEASURED[key], ceiling)


def _rounder(dtype):
    td = ops.torch_dtype(dtype)

    def r16(a):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return t.to(td).to(t.dtype).numpy()
    return r16


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.torch_dtype(dtype)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


# ---- l2s_kv_attention -------------------------------------------------------------------------------------------------------------

SELF_T = 448
SELF_VALID = (1, 2, 63, 64, 65, 447, 448)


def _attend(q, k, v, dtype, *, valid=None, per_clip=False, n_valid=0, kn=None, vn=None, poison=True):
    """Runs the kernel on caches whose rows at or past the valid length (and, with new rows, the row they go to) hold NaN."""
    B, H = q.shape[0], q.shape[1]
    T = k.shape[1]
    vl = np.full(B, n_valid) if valid is None else np.broadcast_to(np.asarray(valid), (B,))
    kc, vc = k.copy(), v.copy()
    if poison:
        for b in range(B):
            lo = vl[b] - 1 if kn is not None else vl[b]
            kc[b, lo:], vc[b, lo:] = np.nan, np.nan
    dq, dk, dv = _dev(q.reshape(B, H * 64), dtype), _dev(kc.reshape(B, T, H * 64), dtype), _dev(vc.reshape(B, T, H * 64), dtype)
    k_before, v_before = _bits(dk), _bits(dv)
    out = torch.full((B, H * 64), float("nan"), device="cuda", dtype=ops.torch_dtype(dtype))
    pos = None
    if valid is not None:
        pos = torch.tensor((vl - 1) if per_clip else [int(vl[0]) - 1], dtype=torch.int32).cuda()
    dkn = _dev(kn.reshape(B, H * 64), dtype) if kn is not None else None
    dvn = _dev(vn.reshape(B, H * 64), dtype) if vn is not None else None
    ops.kv_attention(dq, dk, dv, out, B=B, H=H, pos=pos, pos_stride=1 if per_clip else 0, n_valid=n_valid, k_new=dkn, v_new=dvn,
                     dtype=dtype)
    torch.cuda.synchronize()
    # the caches: the new rows at the device position, every other byte as it was
    k_after, v_after = _bits(dk), _bits(dv)
    if kn is not None:
        for b in range(B):
            assert np.array_equal(k_after[b, vl[b] - 1], _bits(dkn)[b]) and np.array_equal(v_after[b, vl[b] - 1], _bits(dvn)[b])
            k_before[b, vl[b] - 1], v_before[b, vl[b] - 1] = k_after[b, vl[b] - 1], v_after[b, vl[b] - 1]
    assert np.array_equal(k_after, k_before) and np.array_equal(v_after, v_before), "the cache changed outside the appended row"
    return out


def _check_attention(out, ref, dtype, worst):
    got = out.double().cpu().numpy().reshape(ref.shape)
    assert np.isfinite(got).all(), "a row past the valid length was read"
    r16 = _rounder(dtype)
    worst["err"] = max(worst["err"], float(np.abs(got - ref).max()))
    worst["eps"] = max(worst["eps"], float(np.abs(r16(ref) - ref).max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
@pytest.mark.parametrize("H", [2, 6, 20])
def test_kv_attention_self_against_float64(H, dtype):
    B = 3
    q, k, v, kn, vn = R.attention_case(100 + H, B, H, SELF_T, _rounder(dtype))
    worst = {"err": 0.0, "eps": 0.0}
    for valid in SELF_VALID:
        for append in (False, True):
            a = dict(kn=kn, vn=vn) if append else {}
            out = _attend(q, k, v, dtype, valid=valid, **a)
            ref, _, _ = R.kv_attention(q, k, v, np.full(B, valid), *((kn, vn) if append else ()))
            _check_attention(out, ref, dtype, worst)
    # one launch, a position per clip: the clips' lengths are independent of one another
    for vl in ((1, 64, 447), (448, 65, 2), (63, 448, 64)):
        out = _attend(q, k, v, dtype, valid=vl, per_clip=True, kn=kn, vn=vn)
        ref, _, _ = R.kv_attention(q, k, v, np.asarray(vl), kn, vn)
        _check_attention(out, ref, dtype, worst)
    assert worst["err"] <= _bound("attn_" + DNAME[dtype], worst["err"], 4.0 * worst["eps"])


@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
@pytest.mark.parametrize("H", [2, 6, 20])
def test_kv_attention_cross_against_float64(H, dtype):
    B, T = 3, 1500
    q, k, v, _, _ = R.attention_case(200 + H, B, H, T, _rounder(dtype))
    worst = {"err": 0.0, "eps": 0.0}
    for n in (1500, 1001):
        out = _attend(q, k, v, dtype, n_valid=n)
        ref, _, _ = R.kv_attention(q, k, v, np.full(B, n))
        _check_attention(out, ref, dtype, worst)
    assert worst["err"] <= _bound("attn_" + DNAME[dtype], worst["err"], 4.0 * worst["eps"])


@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
def test_kv_attention_bytes_alone_in_batch_and_again(dtype):
    B, H = 3, 6
    q, k, v, kn, vn = R.attention_case(300, B, H, SELF_T, _rounder(dtype))
    vl = (65, 447, 2)
    full = _bits(_attend(q, k, v, dtype, valid=vl, per_clip=True, kn=kn, vn=vn))
    again = _bits(_attend(q, k, v, dtype, valid=vl, per_clip=True, kn=kn, vn=vn))
    assert np.array_equal(full, again)
    for b in range(B):
        s = slice(b, b + 1)
        alone = _bits(_attend(q[s], k[s], v[s], dtype, valid=vl[b], kn=kn[s], vn=vn[s]))
        assert np.array_equal(alone[0], full[b]), b


def test_kv_attention_rejects_what_it_does_not_support():
    z = torch.zeros(1, 64, device="cuda", dtype=torch.float16)
    c = torch.zeros(1, 1501, 64, device="cuda", dtype=torch.float16)
    with pytest.raises(ops.L2SError):
        ops.kv_attention(z, c, c, z, B=1, H=1, n_valid=4)                       # cache_T > 1500
    c = torch.zeros(1, 8, 64, device="cuda", dtype=torch.float16)
    with pytest.raises(ops.L2SError):
        ops.kv_attention(z, c, c, z, B=1, H=1, n_valid=9)                       # more valid rows than the cache has
    with pytest.raises(ops.L2SError):
        ops.kv_attention(z, c, c, z, B=1, H=1, n_valid=4, k_new=z, v_new=z)     # an appended row needs the device position
    w = torch.zeros(1, 21 * 64, device="cuda", dtype=torch.float16)
    c = torch.zeros(1, 8, 21 * 64, device="cuda", dtype=torch.float16)
    with pytest.raises(ops.L2SError):
        ops.kv_attention(w, c, c, w, B=1, H=21, n_valid=4)                      # 64 H > 1280


# ---- l2s_vocab_argmax -------------------------------------------------------------------------------------------------------------

VOCAB_SHAPES = [(333, 128, 3), (320, 128, 1), (51864, 384, 17), (51864, 1280, 33)]
FIRST = 3                    # "the first sampled position" of these cases


class _Vocab:
    def __init__(self, V, d, B, dtype):
        self.V, self.d, self.B, self.dtype = V, d, B, dtype
        x, emb, self.top, self.dup, self.second = R.vocab_case(V + d + B, V, d, B, _rounder(dtype))
        x64 = x.astype(np.float64)
        self.ref = np.concatenate([x64 @ emb[i:i + 8192].astype(np.float64).T for i in range(0, V, 8192)], axis=1)
        # float32 CPU evaluations of the same logits: BLAS over everything, and a k-ordered chain over 256 rows (the planted ones first)
        self.l32 = x.astype(np.float32) @ emb.astype(np.float32).T
        e32 = float(np.abs(self.l32.astype(np.float64) - self.ref).max())
        rows = np.unique(np.concatenate([self.top, self.dup, self.second, np.arange(0, V, max(1, V // 200))]))[:256]
        chain = np.zeros((B, len(rows)), np.float32)
        xs, es = x.astype(np.float32), emb[rows].astype(np.float32)
        for kk in range(d):
            chain += xs[:, kk:kk + 1] * es[:, kk][None, :]
        self.eps_logit = max(e32, float(np.abs(chain.astype(np.float64) - self.ref[:, rows]).max()))
        self.x, self.emb = _dev(x, dtype), _dev(emb, dtype)
        self.work = torch.empty(ops.vocab_argmax_workspace(V, B), device="cuda", dtype=torch.uint8)

    def run(self, forbid=None, begin=None, step=None, dump=False):
        B, V = self.B, self.V
        tok = torch.full((B,), -7, device="cuda", dtype=torch.int32)
        lp = torch.full((B,), float("nan"), device="cuda")
        logits = torch.full((B, V), float("nan"), device="cuda") if dump else None
        m = [None if a is None else torch.from_numpy(a.astype(np.uint8)).cuda() for a in (forbid, begin)]
        st = None if step is None else torch.tensor([step], dtype=torch.int32).cuda()
        ops.vocab_argmax(self.x, self.emb, self.work, tok, lp, B=B, V=V, d=self.d, suppress=m[0], begin_suppress=m[1], step=st,
                         first_step=FIRST, logits=logits, dtype=self.dtype)
        torch.cuda.synchronize()
        return tok.cpu().numpy(), lp.double().cpu().numpy(), None if logits is None else logits.double().cpu().numpy()

    def eps_logprob(self, forbid):
        """|float32 evaluation - float64| of the chosen id's log softmax, never below one float32 ulp at the value's scale."""
        _, lp64, _ = R.masked_argmax(self.ref, forbid)
        allowed = np.flatnonzero(~forbid)
        sub = self.l32[:, allowed]
        top = sub.max(axis=1)
        lp32 = -np.log(np.exp(sub - top[:, None]).sum(axis=1, dtype=np.float32))
        return max(float(np.abs(lp32.astype(np.float64) - lp64).max()), float(2.0 ** -23 * max(1.0, np.abs(lp64).max())))


_VOCAB_PARAMS = [pytest.param(s + (dt,), id=f"V{s[0]}_d{s[1]}_B{s[2]}_{DNAME[dt]}") for s in VOCAB_SHAPES for dt in DTYPES]


@pytest.fixture(scope="module", params=_VOCAB_PARAMS)
def vocab(request):
    """One case (operands, float64 logits, float32 yardsticks) shared by the tests of a (shape, dtype); built once, never changed."""
    return _Vocab(*request.param)


def _mask(V, ids):
    m = np.zeros(V, bool)
    m[np.asarray(ids, dtype=np.int64)] = True
    return m


def test_vocab_argmax_logits_ids_and_logprob(vocab):
    c = vocab
    name = DNAME[c.dtype]
    tok, lp, logits = c.run(dump=True)
    err = float(np.abs(logits - c.ref).max())
    tol = _bound("logit_" + name, err, 4.0 * c.eps_logit)
    assert err <= tol
    # decisive by construction: the planted row leads every id but its exact copy by >= 8 x the logit bound, in every clip
    none = np.zeros(c.V, bool)
    for b in range(c.B):
        _, _, margin = R.masked_argmax(c.ref[b:b + 1], _mask(c.V, [c.dup[b]]))
        assert margin[0] >= 8.0 * 4.0 * c.eps_logit
    ids, lp64, _ = R.masked_argmax(c.ref, none)
    assert np.array_equal(ids, c.top)                       # numpy's first maximum = the smaller id of the tie
    assert np.array_equal(tok, c.top), "an exact tie must go to the smaller id"
    lerr = float(np.abs(lp - lp64).max())
    assert lerr <= _bound("logprob_" + name, lerr, 4.0 * c.eps_logprob(none))
    # run to run, and without the dump
    tok2, lp2, _ = c.run()
    assert np.array_equal(tok2, tok) and np.array_equal(lp2, lp)


def test_vocab_argmax_masks(vocab):
    c = vocab
    name = DNAME[c.dtype]
    # the maximum suppressed: its copy wins; both suppressed: the second planted row, with the log-probability over what is left
    tok, _, _ = c.run(forbid=_mask(c.V, c.top))
    assert np.array_equal(tok, c.dup)
    both = _mask(c.V, np.concatenate([c.top, c.dup]))
    ids, lp64, margin = R.masked_argmax(c.ref, both)
    assert np.array_equal(ids, c.second) and (margin >= 8.0 * 4.0 * c.eps_logit).all()
    tok, lp, _ = c.run(forbid=both)
    assert np.array_equal(tok, c.second)
    lerr = float(np.abs(lp - lp64).max())
    assert lerr <= _bound("logprob_" + name, lerr, 4.0 * c.eps_logprob(both))
    # begin_suppress binds at the first sampled position only
    tok, _, _ = c.run(begin=both, step=FIRST)
    assert np.array_equal(tok, c.second)
    tok, _, _ = c.run(begin=both, step=FIRST + 1)
    assert np.array_equal(tok, c.top)
    tok, _, _ = c.run(forbid=_mask(c.V, c.top), begin=_mask(c.V, c.dup), step=FIRST)
    assert np.array_equal(tok, c.second)
    # all ids but one suppressed (the last id, in the partial tile when V is no multiple of 64): it is chosen with probability 1
    only = ~_mask(c.V, [c.V - 1])
    tok, lp, _ = c.run(forbid=only)
    assert (tok == c.V - 1).all() and np.abs(lp).max() == 0.0
    # nothing allowed: -1, which l2s_whisper_advance reads as eot
    tok, _, _ = c.run(forbid=np.ones(c.V, bool))
    assert (tok == -1).all()


def test_vocab_argmax_rejects_what_it_does_not_support():
    assert ops.vocab_argmax_workspace(65537, 1) == 0 and ops.vocab_argmax_workspace(65536, 1) > 0
    x = torch.zeros(1, 96, device="cuda", dtype=torch.float16)
    e = torch.zeros(10, 96, device="cuda", dtype=torch.float16)
    w = torch.empty(ops.vocab_argmax_workspace(10, 1), device="cuda", dtype=torch.uint8)
    tok, lp = torch.zeros(1, device="cuda", dtype=torch.int32), torch.zeros(1, device="cuda")
    with pytest.raises(ops.L2SError):
        ops.vocab_argmax(x, e, w, tok, lp, B=1, V=10, d=96)                      # d is no multiple of 64
    with pytest.raises(ops.L2SError):
        ops.vocab_argmax(x, e, w[:4], tok, lp, B=1, V=10, d=64)                  # workspace too small


# ---- l2s_whisper_advance ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
@pytest.mark.parametrize("B", [5, 300])
def test_whisper_advance_bookkeeping(B, dtype):
    V, d, n_ctx, n_cols, eot = 50, 64, 6, 5, 7
    rng = np.random.default_rng(B)
    r16 = _rounder(dtype)
    emb = r16(rng.standard_normal((V, d)).astype(np.float32))
    pe = rng.standard_normal((n_ctx, d)).astype(np.float32)
    # clip 0 never ends, clip 1 ends at step 1, clip 2 at step 0, clip 3 sends an id outside the vocabulary at step 2 (= eot), clip 4 a
    # negative one at step 3; the rest end at random steps or not at all.  Tokens drawn after a clip's end must not show anywhere.
    steps = 6
    draw = rng.integers(8, V, size=(steps, B))
    draw[1, 1], draw[0, 2], draw[2, 3], draw[3, 4] = eot, eot, V + 3, -1
    for b in range(5, B):
        if rng.random() < 0.7:
            draw[rng.integers(0, steps), b] = eot
    lps = -rng.random((steps, B)).astype(np.float32)
    st = dict(tokens=np.full((B, n_cols), -9, np.int32), sum_logprob=np.zeros(B, np.float32), lengths=np.zeros(B, np.int32),
              done=np.zeros(B, bool), pos=0)
    dev = dict(tokens=torch.from_numpy(st["tokens"]).cuda(), sum_logprob=torch.zeros(B, device="cuda"),
               lengths=torch.zeros(B, device="cuda", dtype=torch.int32), done=torch.zeros(B, device="cuda", dtype=torch.uint8),
               pos=torch.zeros(1, device="cuda", dtype=torch.int32), n_active=torch.full((1,), -1, device="cuda", dtype=torch.int32))
    demb, dpe = _dev(emb, dtype), torch.from_numpy(pe).cuda()
    for s in range(steps):
        token = torch.from_numpy(draw[s].astype(np.int32)).cuda()
        lp = torch.from_numpy(lps[s]).cuda()
        x_next = torch.full((B, d), 123.0, device="cuda")
        ops.whisper_advance(token, lp, dev["tokens"], dev["sum_logprob"], dev["lengths"], dev["done"], demb, dpe, x_next, dev["pos"],
                            dev["n_active"], B=B, V=V, d=d, eot=eot, dtype=dtype)
        torch.cuda.synchronize()
        want = R.advance(draw[s], lps[s], st["tokens"], st["sum_logprob"], st["lengths"], st["done"], emb, pe, st["pos"], eot)
        assert np.array_equal(token.cpu().numpy(), want["token"])
        assert np.array_equal(dev["tokens"].cpu().numpy(), want["tokens"])              # column pos only; none past the last column
        assert np.array_equal(dev["sum_logprob"].cpu().numpy(), want["sum_logprob"])    # one fp32 add per live step: exact
        assert np.array_equal(dev["lengths"].cpu().numpy(), want["lengths"])
        assert np.array_equal(dev["done"].cpu().numpy().astype(bool), want["done"])
        assert int(dev["pos"].item()) == want["pos"] and int(dev["n_active"].item()) == want["n_active"]
        if want["x_next"] is None:
            assert (x_next == 123.0).all()                                              # no position row left: nothing written
        else:
            assert np.array_equal(x_next.cpu().numpy(), want["x_next"])                 # one fp32 add per element: exact
        st = {k: want[k] for k in st}
    assert st["done"][1] and st["done"][2] and st["done"][3] and st["done"][4] and not st["done"][0]
    assert (st["tokens"][2] == eot).all() and st["lengths"][2] == 0 and st["lengths"][1] == 1
