"""Re-derive the per-layer gate constants of tests/_layer_reference.py (C_FROB, C_ROW) on the CPU.

rho = the largest ratio, either way, between the per-layer errors of two correct 16-bit emulations (accumulation in one
piece vs in 8 K-slices) over all 24 + 12 layers, both dtypes and every checked clip length of the points of
tests/test_layer_taps_gpu.py; the constants are max(2, 1.5 rho).  Inputs as in that derivation: full-strength seed-0
weights, encoder input = the fp32 oracle's post_extract_proj rows of random-pixel clips (600 rows from six 100-frame clips),
conformer input = the fp32 oracle's encoder output, final LayerNorm, x2 repeat, proj_in, rounded to the run's 16-bit type.

  python tools/layer_gate_rho.py            # all point lengths (a few minutes on 8 CPUs)
  python tools/layer_gate_rho.py 100 25     # some of them
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LENGTHS = (100, 73, 40, 37, 25, 600)      # encoder rows of the checked clips of points A, B and C


def main(lengths):
    from lip2speech_unit_amd import ops, weights
    from lip2speech_unit_amd.model_avhubert import MultiTargetAVHubertEncoderModel
    from oracle import avhubert as oa
    from oracle import conformer as oc
    from oracle import stage1 as os1
    from tests import _layer_reference as lr
    model = MultiTargetAVHubertEncoderModel.build_model(dtype=ops.F16)
    sd = weights.synth_state_dict(weights.spec_of(model), seed=0)
    del model
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
    rho = {"fp16": [1.0, 1.0], "bf16": [1.0, 1.0]}
    with torch.no_grad():
        for n in lengths:
            x = X[:n]
            y = oa.transformer_encoder(enc_sd, "w2v_model.encoder", x[None], None)[0].repeat_interleave(2, 0)
            for name, t16 in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
                xin = oc._lin(con_sd, "conformer.proj_in", y.to(t16).float()).to(t16).float()
                for stack, (rf, rr, e, w) in lr.emulation_spread(sd, x, xin, t16).items():
                    print(f"n {n:4d} {name} {stack:4s}: rho Frobenius {rf:.3f}, worst row {rr:.3f}; emulation error max {e:.2e}, "
                          f"worst row max {w:.2e}", flush=True)
                    rho[name] = [max(rho[name][0], rf), max(rho[name][1], rr)]
    rf, rr = max(v[0] for v in rho.values()), max(v[1] for v in rho.values())
    print(f"rho Frobenius {rho['fp16'][0]:.3f} (fp16) / {rho['bf16'][0]:.3f} (bf16) -> C_FROB = {max(2.0, 1.5 * rf):.3g} "
          f"(committed {lr.C_FROB:g})")
    print(f"rho worst row {rho['fp16'][1]:.3f} (fp16) / {rho['bf16'][1]:.3f} (bf16) -> C_ROW = {max(2.0, 1.5 * rr):.3g} "
          f"(committed {lr.C_ROW:g})")


if __name__ == "__main__":
    main(tuple(int(a) for a in sys.argv[1:]) or LENGTHS)
