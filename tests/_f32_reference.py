"""Gate constants of the per-layer fp32 (ops.F32) check, tests/test_f32_models_gpu.py::test_layer_taps_f32_vs_fp64, and their
CPU derivation (tests/test_f32_reference_cpu.py runs it).

Truth is `encoder_fp64` / `conformer_fp64` of tests/_layer_reference.py; the yardstick is `encoder_emulated` /
`conformer_emulated` with t16 = torch.float32, i.e. the same stacks evaluated by torch in float32 (every "round to 16 bits" of
the emulation is the identity).  Rule of tests/_layer_reference.py: rho = the largest ratio, either way, between the per-layer
errors of two correct evaluations (reductions in one piece vs in 8 K-slices: `emulation_spread`), C = max(2, 1.5 * rho).

Derivation (CPU only, before the first GPU run; `derive_rho` below, inputs as tools/layer_gate_rho.py builds them: full-strength
seed-0 weights, encoder input = the fp32 oracle's post_extract_proj rows of random-pixel clips, conformer input = the fp32
oracle's encoder output through the x2 repeat and proj_in), all 24 + 12 layers, encoder rows n of the checked clips:
RHO_TABLE below.
"""
import torch

from tests import _layer_reference as lr

LENGTHS = (100, 73, 40, 37, 25, 600)      # encoder rows of the checked clips of points A, B and C (tests/test_layer_taps_gpu.py)

# n: (enc rho Frobenius, enc rho worst row, conf rho Frobenius, conf rho worst row) as printed by derive_rho on the CPU
# (8 threads, torch 2.x CPU BLAS; 63 s for all six lengths).  The per-layer errors themselves stayed <= 8.2e-7 (Frobenius) /
# 9.6e-7 (worst row) in the encoder and <= 4.7e-7 / 5.4e-7 in the conformer: 5 - 8 fp32 unit roundoffs after 24 / 12 layers.
# The spread is wider than the 16-bit one (1.04) because an fp32 evaluation's error IS its summation order - there is no
# operand rounding that both evaluations share - and it grows with n in the encoder (the attention products sum over n keys).
RHO_TABLE = {
    25: (1.531, 1.535, 1.684, 1.588),
    40: (1.706, 1.774, 1.623, 1.607),
    37: (1.674, 1.687, 1.614, 1.626),
    73: (2.211, 2.287, 1.657, 1.655),
    100: (2.548, 2.831, 1.664, 1.653),
    600: (3.232, 3.424, 1.644, 1.536),
}


def _rho(i):
    return max(v[i] for v in RHO_TABLE.values()) if RHO_TABLE else 1.0


RHO_FROB = max(_rho(0), _rho(2))          # 3.232 (encoder, n = 600)
RHO_ROW = max(_rho(1), _rho(3))           # 3.424 (encoder, n = 600)
C_FROB_F32 = max(2.0, 1.5 * RHO_FROB)     # 4.85
C_ROW_F32 = max(2.0, 1.5 * RHO_ROW)       # 5.14


def stack_inputs(sd, lengths):
    """-> {n: (x [n, 1024] fp32 encoder input rows, xin [2n, 512] fp32 conformer input rows)} from the fp32 oracle."""
    from oracle import avhubert as oa
    from oracle import conformer as oc
    from oracle import stage1 as os1
    enc_sd, con_sd = os1.split_state_dict(sd)
    rows = []
    with torch.no_grad():
        for s in range(-(-max(lengths) // 100)):
            g = torch.Generator().manual_seed(2024 + s)
            video = ((torch.randint(0, 256, (1, 100, 88, 88), generator=g).float() / 255.0 - 0.421) / 0.165).unsqueeze(1)
            taps = {}
            oa.extract_finetune(enc_sd, video, torch.zeros(1, 100, dtype=torch.bool), layers=0, taps=taps)
            rows.append(taps["post_extract_proj"][0])
        X = torch.cat(rows)
        out = {}
        for n in lengths:
            x = X[:n]
            y = oa.transformer_encoder(enc_sd, "w2v_model.encoder", x[None], None)[0].repeat_interleave(2, 0)
            out[n] = (x, oc._lin(con_sd, "conformer.proj_in", y))
    return out


def derive_rho(sd, lengths, enc_layers=24, conf_layers=12):
    """-> {n: (enc rho Frobenius, enc rho worst row, conf rho Frobenius, conf rho worst row)} for float32."""
    table = {}
    with torch.no_grad():
        for n, (x, xin) in stack_inputs(sd, lengths).items():
            sp = lr.emulation_spread(sd, x, xin, torch.float32, enc_layers, conf_layers)
            table[n] = (sp["enc"][0], sp["enc"][1], sp["conf"][0], sp["conf"][1])
            print(f"n {n:4d} float32: enc rho {sp['enc'][0]:.3f} / {sp['enc'][1]:.3f} (errors <= {sp['enc'][2]:.2e} / {sp['enc'][3]:.2e}), "
                  f"conf rho {sp['conf'][0]:.3f} / {sp['conf'][1]:.3f} (errors <= {sp['conf'][2]:.2e} / {sp['conf'][3]:.2e})", flush=True)
    return table
