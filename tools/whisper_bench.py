#!/usr/bin/env python3
"""Times of the on-device Whisper recogniser at base.en's dimensions with seeded random weights: the log-mel front end, the
encoder and one decoder step (graph replay and plain launches) at B = 1 and B = 64, and for the two bandwidth-bound kernels of the
step - l2s_kv_attention over the cross cache, l2s_vocab_argmax over the token embedding - the bytes they have to move over their
time, as a share of the HBM rate a float4 copy reaches on this chip (6.29 TB/s measured, 8.0 TB/s spec).  No threshold, no
parent to compare with (the reference runs Whisper on the CPU and publishes no time): the figures are recorded in DESIGN.md
section 20.

  python tools/whisper_bench.py [--batches 1 64] [--iters 20] [--dtype f16|bf16]

Events around `iters` launches after a warm-up of every shape; 30-s clips of seeded noise.  Prints one JSON line per batch size.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED_TBPS = 6.29


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batches", type=int, nargs="+", default=[1, 64])
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--dtype", default="f16", choices=["f16", "bf16"])
    a = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("whisper_bench measures the MI355X path: no GPU, no figure")
    from lip2speech_unit_amd import ops, weights
    from lip2speech_unit_amd.asr_text import WhisperDecodeConfig
    from lip2speech_unit_amd.whisper import N_CTX_AUDIO, N_SAMPLES, Whisper, WhisperASR, WhisperDims
    dt = ops.BF16 if a.dtype == "bf16" else ops.F16
    dims = WhisperDims.base_en()
    model = Whisper(dims, dtype=dt)
    sd = weights.synth_state_dict(weights.spec_of(model), seed=0)
    sd["encoder.positional_embedding"] = model.encoder.positional_embedding
    model.load_state_dict(sd)
    model.cuda().eval()
    d, H, V = dims.n_text_state, dims.n_text_head, dims.n_vocab

    def timed(fn, iters=a.iters):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for B in a.batches:
        g = torch.Generator(device="cuda").manual_seed(B)
        wav = (torch.randn(B, N_SAMPLES, device="cuda", generator=g) * 3000).to(torch.int16)
        with torch.no_grad():
            feats = model.logmel.features(wav, None, dtype=dt)
            out = {"B": B, "dtype": a.dtype, "frontend_ms": round(timed(lambda: model.logmel.features(wav, None, dtype=dt)), 4),
                   "encoder_ms": round(timed(lambda: model.encode_features(feats, B), max(2, a.iters // 4)), 4)}
            _, enc16 = model.encode_features(feats, B)
            out["cross_kv_ms"] = round(timed(lambda: model.cross_caches(enc16, B)), 4)
            for graph in (True, False):
                asr = WhisperASR(model, WhisperDecodeConfig.english(), graph=graph)
                st = asr._state(B, wav.device)
                for dst, src in zip(st["S"]["cross"], model.cross_caches(enc16, B)):
                    dst.copy_(src)
                model.start(st["S"], 50257)

                def step():
                    st["S"]["pos"].fill_(100)            # a mid-sequence position: 101 valid rows of the self caches
                    asr._replay(st)
                out["step_graph_ms" if graph else "step_plain_ms"] = round(timed(step), 4)
            S = st["S"]
            t16 = ops.torch_dtype(dt)
            q = torch.randn(B, d, device="cuda").to(t16)
            o = torch.empty_like(q)
            ck, cv = S["cross"][0][0], S["cross"][0][1]
            ms = timed(lambda: ops.kv_attention(q, ck, cv, o, B=B, H=H, n_valid=N_CTX_AUDIO, dtype=dt))
            moved = 2.0 * B * N_CTX_AUDIO * d * 2 + 4.0 * B * d
            out["kv_attention_cross"] = {"ms": round(ms, 5), "MB": round(moved / 1e6, 2), "TBps": round(moved / ms / 1e9, 3),
                                         "of_hbm_copy_rate": round(moved / ms / 1e9 / HBM_MEASURED_TBPS, 3)}
            emb = model.packed(wav.device)["emb"]
            tok, lp = torch.empty(B, device="cuda", dtype=torch.int32), torch.empty(B, device="cuda")
            ms = timed(lambda: ops.vocab_argmax(q, emb, S["work"], tok, lp, B=B, V=V, d=d, dtype=dt))
            moved = 2.0 * V * d + 2.0 * B * d + 2 * 12.0 * ((V + 63) // 64) * B
            out["vocab_argmax"] = {"ms": round(ms, 5), "MB": round(moved / 1e6, 2), "TBps": round(moved / ms / 1e9, 3),
                                   "of_hbm_copy_rate": round(moved / ms / 1e9 / HBM_MEASURED_TBPS, 3)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
