#!/usr/bin/env python3
"""The tile boundary of the phase-staggered kernel (csrc/phasegemm_kernel.h: both wave rows levelled for the epilogue, staggered
again behind it), one part per child process - the library reads L2S_PHASE_SLOTS once per process:

    L2S_PHASEGEMM=2 L2S_PHASE_SLOTS=2 check_phasegemm_level.py walk 64|192     7 x 7 tiles, blocks walk four and three tiles
    L2S_PHASEGEMM=2 L2S_PHASE_SLOTS=1 check_phasegemm_level.py uneven          3 x 3 tiles, blocks walk two, one and no tiles
    L2S_PHASE_SLOTS=1 check_phasegemm_level.py ktab                            K-block table: a block walks tiles of different K

walk / uneven: the cases are built by tests/_tapgemm_cases.py and checked by tools/check_tapgemm_matrix.py::run_case (guarded
operands, fp64 oracle, its criteria (a) and (b)); every launch is then repeated REPEATS times from the same start state and must
reproduce the first result bit for bit - a fragment read that is ordered by luck instead of by a counted vmcnt and a barrier shows
as a tile that differs from run to run.  ktab: ResNet's 3 x 3 convolution on a 3 x 3 map against torch's conv2d in fp64, bound as in
tests/test_kernels_gpu.py::test_ktab_conv3x3_small_maps_vs_torch, and the same repeat check."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from lip2speech_unit_amd import _lib, ops  # noqa: E402
from tests import _tapgemm_cases as tc  # noqa: E402
from tools import check_tapgemm_matrix as cm  # noqa: E402

REPEATS = 7
WALK_KS = (64, 192)                                     # one K-tile (the shortest loop) and an odd count (the parity crosses tiles)
WALK_EPIS = ["none", "gelu+mask", "stream32", "res16post+dual+mask", "x32+accum+dual+mask"]
WALK_MN, WALK_SLOTS = (1576, 1784), 2
UNEVEN_KS, UNEVEN_EPIS = (64, 128), ["none", "stream32"]
UNEVEN_MN, UNEVEN_SLOTS = (744, 760), 1
KTAB_SLOTS, KTAB_IMAGES, KTAB_CIN, KTAB_CO, KTAB_HI = 1, 520, 64, 256, 3
PART_ENV = {"walk": dict(L2S_PHASEGEMM="2", L2S_PHASE_SLOTS=str(WALK_SLOTS)),
            "uneven": dict(L2S_PHASEGEMM="2", L2S_PHASE_SLOTS=str(UNEVEN_SLOTS)),
            "ktab": dict(L2S_PHASE_SLOTS=str(KTAB_SLOTS))}


def walk_cases(K):
    M, N = WALK_MN
    _, _, slots, my_n = tc.phase_schedule(M, N, WALK_SLOTS)
    assert slots == 2 and my_n == [[4, 3]] * 7 + [[0, 0]], my_n
    g = tc.g_linear(M, N, K)
    return [tc._case(f"level-walk/linear-K{K}", dt, g, e, tc.PHASE) for dt in tc.DTYPES for e in tc._named(WALK_EPIS)]


def uneven_cases():
    M, N = UNEVEN_MN
    ntiles, chunk, slots, my_n = tc.phase_schedule(M, N, UNEVEN_SLOTS)
    assert (ntiles, chunk, slots) == (9, 2, 1) and my_n == [[2]] * 4 + [[1]] + [[0]] * 3, my_n
    geoms = {K: tc.g_linear(M, N, K) for K in UNEVEN_KS}
    return [tc._case(f"level-uneven/linear-K{K}", dt, geoms[K], e, tc.PHASE)
            for dt in tc.DTYPES for K in UNEVEN_KS for e in tc._named(UNEVEN_EPIS)]


class Repeat:
    """ops.tapgemm, then REPEATS more launches from the same start state of C / C2: every one must equal the first bit for bit."""

    def __init__(self):
        self.real, self.diff, self.launches = ops.tapgemm, [], 0

    def __call__(self, A, W, C, **kw):
        C2 = kw.get("C2")
        start, start2 = C.clone(), (C2.clone() if C2 is not None else None)
        self.real(A, W, C, **kw)
        torch.cuda.synchronize()
        first, first2 = C.clone(), (C2.clone() if C2 is not None else None)
        for i in range(REPEATS):
            C.copy_(start)                               # (an in-place residual is C itself: restored with it)
            if C2 is not None:
                C2.copy_(start2)
            self.real(A, W, C, **kw)
            torch.cuda.synchronize()
            self.launches += 1
            for name, got, want in (("C", C, first), ("C2", C2, first2)):
                if got is not None and not torch.equal(cm.bits(got), cm.bits(want)):
                    n = (cm.bits(got) != cm.bits(want)).sum().item()
                    self.diff.append(f"launch {i + 2}: {n} elements of {name} differ from the first launch")


def run_cases(part, cases):
    lib = _lib.load()
    rep = cm.Report(tc.PHASE)
    hook = Repeat()
    ops.tapgemm = hook
    try:
        for case in cases:
            seen = len(hook.diff)
            cm.run_case(case, lib, tc.PHASE, rep)
            for why in hook.diff[seen:]:
                rep.bad(case, why)
    finally:
        ops.tapgemm = hook.real
    assert hook.launches == REPEATS * len(cases), (hook.launches, len(cases))
    for inst in sorted({k for k, _ in rep.worst}):
        a, b = rep.worst.get((inst, "a")), rep.worst.get((inst, "b"))
        print(f"RATIO {part} " + " ".join(str(x) for x in inst) + f" (a) {a:5.3f} (b) " + ("    -" if b is None else f"{b:5.3f}"))
    return rep.fail


def run_ktab():
    """27 tiles (3 M-tiles x 9 output positions) of 4, 6 or 9 K-blocks; under the slot cap a block walks four of them."""
    from lip2speech_unit_amd.ops import ACT_PRELU, F_RES_PRE
    from lip2speech_unit_amd.resnet import ktab_conv3x3
    Hi, Cin, Co, N = KTAB_HI, KTAB_CIN, KTAB_CO, KTAB_IMAGES
    fail = []
    for dt_name, dt in (("f16", ops.F16), ("bf16", ops.BF16)):
        for res in (False, True):
            t16 = ops.torch_dtype(dt)
            g = torch.Generator().manual_seed(Hi * 100 + Cin + 7 * res)
            x = torch.randn(N, Cin, Hi, Hi, generator=g).to(t16).double()
            w = (torch.randn(Co, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).to(t16).double()
            b, sl = torch.randn(Co, generator=g) * 0.1, torch.rand(Co, generator=g) * 0.4
            tab, Ho, Wo, nblk = ktab_conv3x3(Hi, Hi, Cin, 1, "cuda")
            G = Ho * Wo
            assert G == 9 and sorted(set(tab[:, 0].tolist())) == [4, 6, 9] and -(-N // 256) * G == 27
            r = torch.randn(N, Co, Ho, Wo, generator=g).to(t16).double() if res else None
            ref = F.prelu(F.conv2d(x, w, b.double(), stride=1, padding=1) + (r if res else 0), sl.double())
            rows = lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], -1).contiguous()      # one image = one row
            dA = rows(x).to(t16).cuda()
            dW = w.permute(0, 2, 3, 1).reshape(Co, 9 * Cin).contiguous().to(t16).cuda()
            dR = rows(r).to(t16).cuda() if res else None
            db, ds = b.repeat(G).cuda(), sl.repeat(G).cuda()
            outs = []
            for i in range(1 + REPEATS):
                y = torch.full((N, G * Co), float("nan"), device="cuda", dtype=t16)
                ops.tapgemm(dA, dW, y, M=N, N=Co, Cin=Cin, ntaps=9, lda=Hi * Hi * Cin, ldc=G * Co, groups=G, c_gstride=Co, bias=db,
                            slope=ds, act=ACT_PRELU, R=dR, ldr=G * Co, flags=F_RES_PRE if res else 0, dtype=dt, ktab=tab)
                torch.cuda.synchronize()
                outs.append(y)
            got = outs[0].double().cpu()
            name = f"ktab {dt_name} res={int(res)}"
            if not torch.isfinite(got).all():
                fail.append(f"FAIL {name}: {(~torch.isfinite(got)).sum().item()} elements are not finite")
                continue
            ratio = (got - rows(ref)).abs().max().item() / (cm.TOL[dt_name] * rows(ref).abs().max().item())
            print(f"RATIO {name} (a) {ratio:5.3f}")
            if ratio >= 1.0:
                fail.append(f"FAIL {name}: max err / (tol max|ref|) = {ratio:.3f}")
            for i, y in enumerate(outs[1:]):
                if not torch.equal(cm.bits(y), cm.bits(outs[0])):
                    fail.append(f"FAIL {name}: launch {i + 2} differs from the first in {(cm.bits(y) != cm.bits(outs[0])).sum().item()} elements")
    return fail


def main():
    part = sys.argv[1]
    for name in tc.SWITCHES:                # exactly the part's switches: the kernel under test and its grid
        assert os.environ.get(name) == PART_ENV[part].get(name), (name, os.environ.get(name))
    t0 = time.time()
    if part == "walk":
        K = int(sys.argv[2])
        assert K in WALK_KS
        fail = run_cases(f"walk-K{K}", walk_cases(K))
    elif part == "uneven":
        fail = run_cases("uneven", uneven_cases())
    elif part == "ktab":
        fail = run_ktab()
    else:
        raise ValueError(part)
    print(f"part {' '.join(sys.argv[1:])}: {len(fail)} failures, {time.time() - t0:.1f} s")
    for line in fail:
        print(line)
    sys.exit(1 if fail else 0)


if __name__ == "__main__":
    main()
