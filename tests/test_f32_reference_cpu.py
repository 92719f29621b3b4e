"""CPU derivation of the fp32 per-layer gate constants (tests/_f32_reference.py): the float32 `emulation_spread` of
tests/_layer_reference.py at full depth, the rule C = max(2, 1.5 * rho), and that the float32 evaluation really is an fp32-sized
yardstick (a few unit roundoffs, three orders below the 16-bit emulations)."""
import pytest
import torch

from tests import _f32_reference as fr
from tests import _layer_reference as lr

CHECK_LENGTHS = (25, 100)          # two of the six derivation lengths (the whole table takes a minute: fr.derive_rho)


@pytest.fixture(scope="module")
def sd():
    from lip2speech_unit_amd import ops, weights
    from lip2speech_unit_amd.model_avhubert import MultiTargetAVHubertEncoderModel
    model = MultiTargetAVHubertEncoderModel.build_model(dtype=ops.F16)
    out = weights.synth_state_dict(weights.spec_of(model), seed=0)
    del model
    return out


def test_constants_follow_the_rule():
    assert set(fr.RHO_TABLE) == set(fr.LENGTHS)
    assert fr.RHO_FROB == max(max(v[0], v[2]) for v in fr.RHO_TABLE.values())
    assert fr.RHO_ROW == max(max(v[1], v[3]) for v in fr.RHO_TABLE.values())
    assert fr.C_FROB_F32 == max(2.0, 1.5 * fr.RHO_FROB) and fr.C_ROW_F32 == max(2.0, 1.5 * fr.RHO_ROW)
    assert 2.0 <= fr.C_FROB_F32 < 6.0 and 2.0 <= fr.C_ROW_F32 < 6.0


def test_float32_spread_rederived(sd):
    """Re-derives rho at two lengths.  The float32 errors depend on the CPU BLAS' own summation order (threads, vector width), so
    the re-derived spread is compared with the recorded one within a factor, and must stay under the recorded constants."""
    table = fr.derive_rho(sd, CHECK_LENGTHS)
    for n, got in table.items():
        want = fr.RHO_TABLE[n]
        print(f"\nn {n}: re-derived rho {tuple(round(g, 3) for g in got)}, recorded {want}")
        for g, w in zip(got, want):
            assert 1.0 <= g <= 1.5 * w + 0.5, (n, got, want)
        # at these lengths the rule's own constant stays under the recorded (all-lengths) one
        assert max(2.0, 1.5 * max(got[0], got[2])) <= 1.5 * fr.C_FROB_F32 and max(2.0, 1.5 * max(got[1], got[3])) <= 1.5 * fr.C_ROW_F32


def test_float32_emulation_is_fp32_sized(sd):
    """t16 = float32 turns every rounding point of the emulation into the identity: its per-layer error against fp64 is a few
    2^-24, not 2^-11."""
    x, xin = fr.stack_inputs(sd, (25,))[25]
    with torch.no_grad():
        enc = lr.layer_errors(lr.encoder_emulated(sd, x, torch.float32, 3), lr.encoder_fp64(lr.sd64(sd, lr.ENC), x, 3))
        conf = lr.layer_errors(lr.conformer_emulated(sd, xin, torch.float32, 3), lr.conformer_fp64(lr.sd64(sd, lr.CONF), xin, 3))
    for e, w, _ in enc + conf:
        assert 2.0 ** -27 < e < 2.0 ** -19 and e <= w < 2.0 ** -18, (e, w)
