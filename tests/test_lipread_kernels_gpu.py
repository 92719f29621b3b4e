"""The three beam-step kernels of csrc/s2s_decode.hip on the device, each against float64 (tests/_s2s_reference.py):
l2s_beam_attention, l2s_beam_select, l2s_beam_advance.

Bounds.  Attention: 8 x the largest error measured on an MI355X over the cases of this file (MEASURED below), capped by a ceiling
computed on the CPU that no measurement can loosen: 4 x the error of the float64 result rounded once to the 16-bit output type.
The smaller of the two holds.  Selection: the candidates (slot, token) must be exact - the crafted scores are >= 1e-3 apart or
exactly tied - and the fp32 scores lie within SELECT_TOL of float64 (derivation at SELECT_TOL).  Bookkeeping: exact.  Every test
prints its figure as `MEASURE <key> <value>` before it asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import ops  # noqa: E402
from tests import _s2s_reference as R  # noqa: E402

DTYPES = [ops.F16, ops.BF16]
DNAME = {ops.F16: "f16", ops.BF16: "bf16"}
# largest |device - float64| seen on an MI355X, per quantity (MEASURE lines of this file): half an ulp of the 16-bit output at
# |out| in [2, 4) (the one-key cases, where the output is a value row itself) - the final rounding
MEASURED = {"attn_f16": 9.76e-4, "attn_bf16": 7.81e-3}


def _bound(key, value, ceiling):
    print(f"MEASURE {key} {value:.3e} ceiling {ceiling:.3e}")
    return min(8.0 * MEASURED[key], ceiling)


def _r16(a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(ops.torch_dtype(dtype)).to(t.dtype).numpy()


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.torch_dtype(dtype)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def _check(out, ref, dtype):
    got = out.double().cpu().numpy().reshape(ref.shape)
    assert np.isfinite(got).all(), "a row that must not be read was read"
    err = float(np.max(np.abs(got - ref)))
    ceiling = 4.0 * float(np.max(np.abs(_r16(ref, dtype) - ref)))
    assert err <= _bound("attn_" + DNAME[dtype], err, ceiling), (err, ceiling)


# ---- l2s_beam_attention -----------------------------------------------------------------------------------------------------------

L_MAX = 136
POSITIONS = (0, 1, 33, 65, 130)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("hd", [64, 128, 192])
@pytest.mark.parametrize("beam", [1, 3, 5, 64])
def test_beam_attention_self(hd, beam, dtype):
    """Self form: three clips (all slots live; beam - 2 live; finished), random ancestor tables (duplicated and permuted parents,
    the other half of the double buffer holds different parents), every cache row at or past p NaN."""
    H, B, L = 2, 3, L_MAX
    W = H * hd
    rng = np.random.default_rng(100 * hd + beam)
    q = _r16(rng.normal(0, 1.0, (B, beam, W)) * hd ** -0.5, dtype)
    kn, vn = _r16(rng.normal(0, 1.0, (B, beam, W)), dtype), _r16(rng.normal(0, 1.0, (B, beam, W)), dtype)
    kc, vc = _r16(rng.normal(0, 1.0, (B, beam, L, W)), dtype), _r16(rng.normal(0, 1.0, (B, beam, L, W)), dtype)
    anc = rng.integers(0, beam, (2, B, beam, L))
    n_live = np.array([beam, max(1, beam - 2), beam])
    finished = np.array([0, 0, 1])
    dq, dkn, dvn = _dev(q.reshape(B * beam, W), dtype), _dev(kn.reshape(B * beam, W), dtype), _dev(vn.reshape(B * beam, W), dtype)
    danc = torch.from_numpy(anc).to(torch.int16).cuda()
    dlive, dfin = torch.from_numpy(n_live).to(torch.int32).cuda(), torch.from_numpy(finished).to(torch.uint8).cuda()
    for p in POSITIONS:
        kcp, vcp = kc.copy(), vc.copy()
        kcp[:, :, p:], vcp[:, :, p:] = np.nan, np.nan
        dk, dv = _dev(kcp, dtype), _dev(vcp, dtype)
        k_before, v_before = _bits(dk), _bits(dv)
        out = torch.full((B * beam, W), float("nan"), device="cuda", dtype=ops.torch_dtype(dtype))
        step = torch.tensor([p], dtype=torch.int32).cuda()
        ops.beam_attention(dq, dk, dv, out, B=B, beam=beam, H=H, hd=hd, k_new=dkn, v_new=dvn, anc=danc, step=step, n_live=dlive,
                           finished=dfin, dtype=dtype)
        torch.cuda.synchronize()
        ref = R.beam_attention_self(q, kcp.copy(), vcp.copy(), kn, vn, anc[p & 1], p, H, n_live=n_live, finished=finished)
        _check(out, ref, dtype)
        k_after, v_after = _bits(dk), _bits(dv)
        for b in range(B):
            for i in range(beam):
                if not finished[b] and i < n_live[b]:        # the new row lands at (b, i, p) ...
                    assert np.array_equal(k_after[b, i, p], _bits(dkn).reshape(B, beam, W)[b, i])
                    assert np.array_equal(v_after[b, i, p], _bits(dvn).reshape(B, beam, W)[b, i])
                    k_before[b, i, p], v_before[b, i, p] = k_after[b, i, p], v_after[b, i, p]
        assert np.array_equal(k_after, k_before) and np.array_equal(v_after, v_before), "a cache byte changed outside the new rows"
        got = out.double().cpu().numpy().reshape(B, beam, W)
        assert not got[2].any() and not got[1, n_live[1]:].any(), "dead slots write zeros"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("hd", [64, 128, 192])
@pytest.mark.parametrize("beam", [1, 3, 5, 64])
def test_beam_attention_cross(hd, beam, dtype):
    """Cross form: one cache per clip shared by its slots, valid lengths 1, 7, 64, 65, 200 mixed in one batch with a finished clip,
    the encoder's padded rows NaN."""
    H, T = 2, 200
    lens = np.array([1, 7, 64, 65, 200, 50])
    finished = np.array([0, 0, 0, 0, 0, 1])
    B, W = len(lens), H * hd
    rng = np.random.default_rng(200 * hd + beam)
    q = _r16(rng.normal(0, 1.0, (B, beam, W)) * hd ** -0.5, dtype)
    kc, vc = _r16(rng.normal(0, 1.0, (B, T, W)), dtype), _r16(rng.normal(0, 1.0, (B, T, W)), dtype)
    for b, n in enumerate(lens):
        kc[b, n:], vc[b, n:] = np.nan, np.nan
    n_live = np.array([beam, max(1, beam - 1), beam, beam, beam, beam])
    dk, dv = _dev(kc, dtype), _dev(vc, dtype)
    k_before, v_before = _bits(dk), _bits(dv)
    out = torch.full((B * beam, W), float("nan"), device="cuda", dtype=ops.torch_dtype(dtype))
    ops.beam_attention(_dev(q.reshape(B * beam, W), dtype), dk, dv, out, B=B, beam=beam, H=H, hd=hd,
                       enc_lens=torch.from_numpy(lens).to(torch.int32).cuda(), n_live=torch.from_numpy(n_live).to(torch.int32).cuda(),
                       finished=torch.from_numpy(finished).to(torch.uint8).cuda(), dtype=dtype)
    torch.cuda.synchronize()
    _check(out, R.beam_attention_cross(q, kc, vc, lens, H, n_live=n_live, finished=finished), dtype)
    assert np.array_equal(_bits(dk), k_before) and np.array_equal(_bits(dv), v_before), "the cross caches are read only"


def test_beam_attention_rejects():
    q = torch.zeros(4, 128, dtype=torch.float16).cuda()
    kc = torch.zeros(1, 8, 128, dtype=torch.float16).cuda()
    lens = torch.ones(1, dtype=torch.int32).cuda()
    with pytest.raises(ops.L2SError):          # heads 32 wide
        ops.beam_attention(q, kc, kc.clone(), q.clone(), B=1, beam=4, H=4, hd=32, enc_lens=lens)
    with pytest.raises(ops.L2SError):          # neither form
        ops.beam_attention(q, kc, kc.clone(), q.clone(), B=1, beam=4, H=2, hd=64)


# ---- l2s_beam_select --------------------------------------------------------------------------------------------------------------

def select_tol(V, s):
    """fp32 against float64 for a compared (top) candidate of score s: y = x / T, y - m, lp and lp + cum are one rounding each at a
    scale of at most |s| + 10 (|cum| < 1, the row's log-sum-exp < ln V < 10): 4 x 2 u (|s| + 10) with a factor 2 of slack; the
    exponentials (2 ulp each) and the sum of V terms (64 lane sums of V / 64 terms and six butterfly steps) give a relative
    (V / 64 + 6 + 2) u on the sum, absolute after the logarithm; the logarithm itself 2 ulp of a value < 10.  The floor logits near
    -100 do not enter: they are never compared and their exponentials vanish."""
    u = 2.0 ** -24
    return (V / 64 + 8 + 2 * 10) * u + 8 * u * (np.abs(s) + 10.0)


SPACING = 0.2
DELTA = SPACING / 130.0          # 1.54e-3


def _crafted(B, beam, V, seed, temperature):
    """Logits whose finite scores are >= DELTA = 1.54e-3 apart whatever the step rule.  Every row of a clip is a permutation of one
    base row (a random floor in [-100, -90] and 4 beam + 8 highs 0.2 apart), so all rows share one log-sum-exp; slot r's cumulative
    score is an even multiple of DELTA below zero (distinct per slot, < 130 DELTA = one spacing in all), so two candidates differ by
    0.2 j + 2 DELTA m, never closer than 2 DELTA; the unk penalty UNK_PENALTY = 0.4 + DELTA puts unk on the odd multiples."""
    rng = np.random.default_rng(seed)
    n_hi = min(4 * beam + 8, V - 2)
    logits = np.empty((B, beam, V))
    for b in range(B):
        base = rng.uniform(-100.0, -90.0, V)
        base[:n_hi] = -SPACING * np.arange(n_hi)
        for r in range(beam):
            row = base[rng.permutation(V)]
            if r == 0:                           # slot 0: pad holds the best value, unk the second, eos the third
                for tok, j in ((R.PAD, 0), (R.UNK, 1), (R.EOS, 2)):
                    at = int(np.where(row == base[j])[0][0])
                    row[[tok, at]] = row[[at, tok]]
            logits[b, r] = row
    cum = np.stack([np.stack([-2.0 * DELTA * rng.permutation(64)[:beam] for _ in range(B)]) for _ in range(2)])
    return (logits * temperature).astype(np.float32), cum.astype(np.float32)


UNK_PENALTY = 2 * SPACING + DELTA


def _run_select(logits, cum, step, max_len, n_live, finished, beam, V, ldl, **kw):
    B = logits.shape[0]
    K = 2 * beam
    dl = torch.full((B * beam, ldl), float("nan"), dtype=torch.float32)
    dl[:, :V] = torch.from_numpy(logits.reshape(B * beam, V))
    sc = torch.full((B, K), 7.0, dtype=torch.float32).cuda()
    sl, tk = torch.full((B, K), -7, dtype=torch.int32).cuda(), torch.full((B, K), -7, dtype=torch.int32).cuda()
    ops.beam_select(dl.cuda(), torch.from_numpy(cum).cuda(), torch.tensor([step], dtype=torch.int32).cuda(),
                    torch.tensor(max_len, dtype=torch.int32).cuda(), sc, sl, tk, B=B, beam=beam, V=V, pad=R.PAD, unk=R.UNK, eos=R.EOS,
                    n_live=None if n_live is None else torch.tensor(n_live, dtype=torch.int32).cuda(),
                    finished=None if finished is None else torch.tensor(finished, dtype=torch.uint8).cuda(), ldl=ldl, **kw)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), sl.cpu().numpy(), tk.cpu().numpy()


@pytest.mark.parametrize("V", [36, 1004, 4099])
@pytest.mark.parametrize("beam", [1, 2, 5, 50, 64])
def test_beam_select(V, beam):
    """V < 2 beam + 2 is refused.  Steps 0 (slot 0 only, eos forbidden by min_len), 1 (below min_len = 2), 3 (free), 5 (>= max_len of clip 1: eos only) with the
    unk penalty, a planted NaN logit and a NaN row, live-slot counts and a finished clip."""
    if V < 2 * beam + 2:
        assert ops.beam_select_workspace(V, beam) == 0
        with pytest.raises(ops.L2SError):
            _run_select(np.zeros((1, beam, V), np.float32), np.zeros((2, 1, beam), np.float32), 0, [4], None, None, beam, V, 40)
        return
    B, temperature, unk_penalty, min_len = 3, 1.25, UNK_PENALTY, 2
    ldl = (V + 7) // 8 * 8
    logits, cum = _crafted(B, beam, V, 1000 * V + beam, temperature)
    logits[0, 0, 5] = np.nan                                    # a NaN logit: its whole row is -inf, as after torch's log_softmax
    if beam > 1:
        logits[1, beam - 1, :] = np.nan
    max_len, n_live, finished = [9, 5, 9], [beam, max(1, beam - 1), beam], [0, 0, 1]
    worst = 0.0
    for step in (0, 1, 3, 5):
        sc, sl, tk = _run_select(logits, cum, step, max_len, n_live, finished, beam, V, ldl, min_len=min_len, temperature=temperature,
                                 unk_penalty=unk_penalty)
        assert (sc[2] == 7.0).all() and (sl[2] == -7).all(), "a finished clip's outputs are left alone"
        for b in range(2):
            rs, rl, rt = R.beam_select(logits[b].astype(np.float64), cum[step & 1, b], step, max_len[b], beam, n_live=n_live[b],
                                       min_len=min_len, temperature=temperature, unk_penalty=unk_penalty, extra=1)
            fin = np.isfinite(rs)
            gaps = rs[:-1][fin[1:]] - rs[1:][fin[1:]]
            assert gaps.size == 0 or gaps.min() >= 1e-3, "the crafted case lost its gaps"
            assert np.array_equal(sl[b], rl[:-1]) and np.array_equal(tk[b], rt[:-1]), (V, beam, step, b)
            assert np.array_equal(np.isfinite(sc[b]), fin[:-1])
            f = fin[:-1]
            if f.any():
                err = np.abs(sc[b][f] - rs[:-1][f])
                tol = select_tol(V, rs[:-1][f])
                worst = max(worst, float(np.max(err / tol)))
                assert (err <= tol).all(), (err.max(), tol.min())
    print(f"MEASURE select_err_over_tol_V{V}_beam{beam} {worst:.3e}")


@pytest.mark.parametrize("beam", [2, 5])
def test_beam_select_ties_go_to_the_smaller_flat_index(beam):
    """Rows with identical logits and identical cumulative scores, and equal logits inside a row: exact fp32 ties."""
    V, B = 36, 1
    rng = np.random.default_rng(beam)
    row = rng.permutation(V).astype(np.float32) * 0.25
    row[7] = row[9] = 20.0                                      # a tie inside the row
    logits = np.broadcast_to(row, (B, beam, V)).copy()
    cum = np.full((2, B, beam), -1.5, dtype=np.float32)
    sc, sl, tk = _run_select(logits, cum, 3, [9], [beam], [0], beam, V, 40)
    rs, rl, rt = R.beam_select(logits[0].astype(np.float64), cum[1, 0], 3, 9, beam, n_live=beam)
    assert np.array_equal(sl[0], rl) and np.array_equal(tk[0], rt)
    flat = sl[0].astype(np.int64) * V + tk[0]
    assert (np.diff(sc[0]) <= 0).all() and all(flat[i] < flat[i + 1] for i in range(2 * beam - 1) if sc[0][i] == sc[0][i + 1])
    assert sc[0][0] == sc[0][1] and (flat[0], flat[1]) == (7, 9)


# ---- l2s_beam_advance -------------------------------------------------------------------------------------------------------------

def _advance_case(beam, L, V, d, dtype, scripts, max_len, pre_finished, lenpen, normalize):
    """scripts[b] = list of steps, each a (score [K], slot [K], token [K]) candidate list; runs them through the kernel and the
    restatement side by side and compares every table after every step."""
    B, K = len(scripts), 2 * beam
    rng = np.random.default_rng(5)
    emb = _r16(rng.normal(0, 1, (V, d)), dtype)
    pos = rng.normal(0, 1, (L, d)).astype(np.float32)
    scale = 1.75
    i32, f32 = torch.int32, torch.float32
    z = dict(device="cuda")
    S = {"tokens": torch.full((2, B, beam, L), R.PAD, dtype=i32, **z), "anc": torch.zeros(2, B, beam, L, dtype=torch.int16, **z),
         "scores": torch.zeros(2, B, beam, dtype=f32, **z), "n_live": torch.full((B,), beam, dtype=i32, **z),
         "finished": torch.tensor(pre_finished, dtype=torch.uint8, **z), "parents": torch.zeros(B, beam, dtype=i32, **z),
         "hyp_tokens": torch.full((B, beam, L), R.PAD, dtype=i32, **z), "hyp_len": torch.zeros(B, beam, dtype=i32, **z),
         "hyp_score": torch.zeros(B, beam, dtype=f32, **z), "nhyp": torch.zeros(B, dtype=i32, **z),
         "out_tokens": torch.full((B, beam, L), R.PAD, dtype=i32, **z), "out_len": torch.zeros(B, beam, dtype=i32, **z),
         "out_score": torch.full((B, beam), float("-inf"), dtype=f32, **z), "x": torch.full((B * beam, d), float("nan"), dtype=f32, **z),
         "step": torch.zeros(1, dtype=i32, **z), "n_active": torch.zeros(1, dtype=i32, **z)}
    S["tokens"][:, :, :, 0] = R.EOS
    S["anc"][:, :, :, 0] = torch.arange(beam, dtype=torch.int16, **z).view(1, 1, beam)
    dmax = torch.tensor(max_len, dtype=i32, **z)
    demb, dpos = _dev(emb, dtype), torch.from_numpy(pos).cuda()
    refs = [R.ClipState(beam, L) for _ in range(B)]
    for b in range(B):
        refs[b].finished = bool(pre_finished[b])
    n_steps = max(len(s) for s in scripts)
    for st in range(n_steps):
        cs, cl, ct = np.zeros((B, K), np.float32), np.zeros((B, K), np.int32), np.zeros((B, K), np.int32)
        for b in range(B):
            sc, sl, tk = scripts[b][min(st, len(scripts[b]) - 1)]
            cs[b], cl[b], ct[b] = sc, sl, tk
        x_before = S["x"].clone()
        ops.beam_advance(torch.from_numpy(cs).cuda(), torch.from_numpy(cl).cuda(), torch.from_numpy(ct).cuda(), S["tokens"], S["anc"],
                         S["scores"], S["n_live"], S["finished"], S["parents"], S["hyp_tokens"], S["hyp_len"], S["hyp_score"], S["nhyp"],
                         S["out_tokens"], S["out_len"], S["out_score"], dmax, demb, dpos, S["x"], S["step"], S["n_active"], B=B, beam=beam,
                         V=V, d=d, eos=R.EOS, pad=R.PAD, embed_scale=scale, lenpen=lenpen, normalize_scores=normalize, dtype=dtype)
        torch.cuda.synchronize()
        nxt = (st + 1) & 1
        assert int(S["step"].item()) == st + 1
        for b in range(B):
            ref = refs[b]
            was = ref.finished
            if not was:
                assert ref.step == st
            new = R.beam_advance(ref, cs[b].astype(np.float64), cl[b], ct[b], max_len[b], lenpen=lenpen, normalize=normalize)
            if was:
                ref.step = st + 1
                assert torch.equal(S["x"][b * beam:(b + 1) * beam].isnan(), x_before[b * beam:(b + 1) * beam].isnan())
            assert bool(S["finished"][b].item()) == ref.finished, (st, b)
            assert int(S["nhyp"][b].item()) == len(ref.hyps), (st, b)
            assert int(S["n_live"][b].item()) == ref.n_live or was, (st, b)
            if not ref.finished:
                n = ref.n_live
                assert np.array_equal(S["tokens"][nxt, b, :n, :st + 2].cpu().numpy(), ref.tokens[:n, :st + 2]), (st, b)
                assert np.array_equal(S["anc"][nxt, b, :n, :st + 2].cpu().numpy(), ref.anc[:n, :st + 2]), (st, b)
                assert np.array_equal(S["parents"][b, :n].cpu().numpy(), ref.parents[:n])
                assert np.array_equal(S["scores"][nxt, b, :n].cpu().numpy(), ref.scores[:n].astype(np.float32))
                want = scale * emb[np.array(new)] + pos[st + 1].astype(np.float64)
                got = S["x"][b * beam:b * beam + n].double().cpu().numpy()
                assert np.max(np.abs(got - want)) <= 2.0 ** -22 * (1.0 + np.max(np.abs(want)))
            elif ref.out is not None:
                for i, (toks, score) in enumerate(ref.out):
                    assert int(S["out_len"][b, i].item()) == len(toks)
                    assert S["out_tokens"][b, i].cpu().tolist() == toks + [R.PAD] * (L - len(toks)), (st, b, i)
                    assert abs(float(S["out_score"][b, i].item()) - score) <= 2.0 ** -21 * (1.0 + abs(score))
        assert int(S["n_active"].item()) == sum(0 if r.finished else 1 for r in refs)
    return S, refs


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("beam", [1, 3, 64])
def test_beam_advance_scripted(beam, dtype):
    """Four clips over six steps of scripted candidates: eos at rank < beam (finalised) and at rank >= beam (skipped), a clip that
    collects `beam` hypotheses, a clip that runs into max_len, a clip finished before the first step; equal final scores."""
    V, d, L, K = 300, 64, 16, 2 * beam
    rng = np.random.default_rng(beam)

    def cands(eos_ranks, all_eos=False):
        tk = rng.integers(4, V, K)
        tk[list(eos_ranks)] = R.EOS
        if all_eos:
            tk[:] = R.EOS
        sc = -np.sort(rng.uniform(0.5, 9.0, K))
        sc = np.round(sc * 64) / 64                              # exact in fp32
        return sc.astype(np.float32), rng.integers(0, beam, K), tk
    late = [K - 1] if beam > 1 else []
    scripts = [
        # eos at rank 0 every step from step 1 on: collects hypotheses (and `beam` of them at once when beam = 1)
        [cands([])] + [cands([0] + late) for _ in range(5)],
        # eos only at ranks >= beam: never finalised; runs into max_len = 3, where every candidate is eos
        [cands(late), cands(late), cands(late), cands([], all_eos=True)],
        # finished before the first step: inert
        [cands([0])],
        # every one of the first beam is eos at step 2 with equal scores: `beam` hypotheses at once, ties in finalisation order
        [cands([]), cands([]), (np.full(K, -2.0, np.float32), rng.integers(0, beam, K), np.where(np.arange(K) < beam, R.EOS, 9))],
    ]
    S, refs = _advance_case(beam, L, V, d, dtype, scripts, max_len=[9, 3, 9, 9], pre_finished=[0, 0, 1, 0], lenpen=1.0, normalize=True)
    assert refs[1].finished and refs[3].finished and len(refs[3].out) == beam and int(S["nhyp"][2].item()) == 0
    assert [len(h[0]) for h in refs[3].out] == [3] * beam


def test_beam_advance_without_normalisation_and_lenpen():
    beam, K = 2, 4
    tk = np.array([R.EOS, 7, R.EOS, 8])
    scripts = [[(np.array([-1, -2, -3, -4], np.float32), np.zeros(K, np.int64), np.array([5, 6, 7, 8]))] +
               [(np.array([-1.5, -2, -3, -4], np.float32), np.array([1, 0, 0, 1]), tk)] * 3]
    for lenpen, normalize in ((0.5, True), (1.0, False)):
        _advance_case(beam, 8, 40, 32, ops.F16, scripts, max_len=[6], pre_finished=[0], lenpen=lenpen, normalize=normalize)
