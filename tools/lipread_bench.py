#!/usr/bin/env python3
"""Times of the on-device lip-reader beam search at the large fine-tuning configuration (decoder 1024 wide, 9 layers, 8 heads of
128, V = 1004, beam 50, 100 encoder rows per clip, B in {1, 8}) with seeded random weights, next to a plain PyTorch-ROCm fp16
restatement of the same step on the same GPU that keeps fairseq's data flow: K/V caches of every layer reordered with
index_select each step, the encoder K/V replicated beam times, log_softmax + topk over beam * V.  No threshold: the figures are
recorded in DESIGN.md section 21.

  python tools/lipread_bench.py [--batches 1 8] [--steps 64] [--repeats 5] [--dtype f16|bf16]

Both sides run `steps` steps of a search that cannot end early (min_len = steps), after a warm-up run of every shape; device
events around the steps, the two sides alternating, `repeats` times; the median is reported with the spread.  ms_per_step,
tokens_per_s = B * beam * 1000 / ms_per_step (rows advanced per second) and the launches of one step (ops launches counted by the
profiler hook on the device side, kernels seen by torch.profiler on the PyTorch side, None when it is unavailable).  Invariants
checked: every hypothesis of the device search ends in eos, has steps + 1 tokens and the scores come best first."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Count:
    detail = False

    def __init__(self):
        self.records = []


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--dtype", default="f16", choices=["f16", "bf16"])
    p.add_argument("--t-enc", type=int, default=100)
    a = p.parse_args(argv)
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("lipread_bench measures the MI355X path: no GPU, no figure")
    import types

    from lip2speech_unit_amd import ops
    from lip2speech_unit_amd.lip_reader import EOS, PAD, BeamSearchConfig, DecoderConfig, LipReader, TransformerDecoder
    dt = ops.BF16 if a.dtype == "bf16" else ops.F16
    t16 = ops.torch_dtype(dt)
    cfg = DecoderConfig()
    V, beam, d, H, T = 1004, 50, cfg.decoder_embed_dim, cfg.decoder_attention_heads, a.t_enc
    torch.manual_seed(0)
    dec = TransformerDecoder(cfg, V, dtype=dt)
    with torch.no_grad():
        torch.nn.init.normal_(dec.embed_tokens.weight, 0, d ** -0.5)
        dec.layer_norm.weight.mul_(4.0)
    dec.cuda().eval()
    steps = a.steps
    # max_len_b = steps and min_len = steps: eos is forbidden before the last step and forced at it - exactly steps + 1 steps
    search = BeamSearchConfig(beam=beam, max_len_a=0.0, max_len_b=steps, min_len=steps, nbest=beam)
    reader = LipReader(types.SimpleNamespace(decoder=dec), None, search, graph=True, cache_bytes=32 << 30)

    # ---- the PyTorch restatement (fairseq's data flow) ------------------------------------------------------------------------
    L = [{k: v.detach().to("cuda", t16) for k, v in lay.state_dict().items()} for lay in dec.layers]
    emb = dec.embed_tokens.weight.detach().to("cuda", t16)
    lnw, lnb = dec.layer_norm.weight.detach().to("cuda", t16), dec.layer_norm.bias.detach().to("cuda", t16)
    pos = dec.position_rows(steps + 8, "cuda").to(t16)
    hd = d // H

    def torch_run(enc, n_steps, count_only=False):
        B = enc.shape[0]
        M = B * beam
        encr = enc.to(t16).repeat_interleave(beam, 0)                          # fairseq: encoder_out reordered to bsz * beam
        cross = [(F.linear(encr, w["encoder_attn.k_proj.weight"], w["encoder_attn.k_proj.bias"]).view(M, T, H, hd).transpose(1, 2),
                  F.linear(encr, w["encoder_attn.v_proj.weight"], w["encoder_attn.v_proj.bias"]).view(M, T, H, hd).transpose(1, 2)) for w in L]
        kc = [torch.empty(M, H, 0, hd, device="cuda", dtype=t16) for _ in L]
        vc = [torch.empty(M, H, 0, hd, device="cuda", dtype=t16) for _ in L]
        tok = torch.full((M,), EOS, device="cuda", dtype=torch.long)
        scores = torch.zeros(B, beam, device="cuda")
        base = (torch.arange(B, device="cuda") * beam)[:, None]
        for st in range(n_steps):
            x = emb[tok] + pos[st]
            for i, w in enumerate(L):
                h = F.layer_norm(x, (d,), w["self_attn_layer_norm.weight"], w["self_attn_layer_norm.bias"])
                q = F.linear(h, w["self_attn.q_proj.weight"], w["self_attn.q_proj.bias"]).view(M, H, 1, hd)
                kc[i] = torch.cat([kc[i], F.linear(h, w["self_attn.k_proj.weight"], w["self_attn.k_proj.bias"]).view(M, H, 1, hd)], 2)
                vc[i] = torch.cat([vc[i], F.linear(h, w["self_attn.v_proj.weight"], w["self_attn.v_proj.bias"]).view(M, H, 1, hd)], 2)
                att = F.scaled_dot_product_attention(q, kc[i], vc[i]).reshape(M, d)
                x = x + F.linear(att, w["self_attn.out_proj.weight"], w["self_attn.out_proj.bias"])
                h = F.layer_norm(x, (d,), w["encoder_attn_layer_norm.weight"], w["encoder_attn_layer_norm.bias"])
                q = F.linear(h, w["encoder_attn.q_proj.weight"], w["encoder_attn.q_proj.bias"]).view(M, H, 1, hd)
                att = F.scaled_dot_product_attention(q, cross[i][0], cross[i][1]).reshape(M, d)
                x = x + F.linear(att, w["encoder_attn.out_proj.weight"], w["encoder_attn.out_proj.bias"])
                h = F.layer_norm(x, (d,), w["final_layer_norm.weight"], w["final_layer_norm.bias"])
                x = x + F.linear(F.relu(F.linear(h, w["fc1.weight"], w["fc1.bias"])), w["fc2.weight"], w["fc2.bias"])
            lp = F.log_softmax(F.linear(F.layer_norm(x, (d,), lnw, lnb), emb).float(), -1)
            lp[:, PAD] = float("-inf")
            lp[:, EOS] = float("-inf")
            lp = lp.view(B, beam, V) + scores[:, :, None]
            cs, ci = torch.topk((lp[:, :1] if st == 0 else lp).reshape(B, -1), 2 * beam)
            scores, parent, tok = cs[:, :beam], ci[:, :beam] // V, (ci[:, :beam] % V).reshape(-1)
            order = (parent + base).reshape(-1)
            for i in range(len(L)):                                         # reorder_incremental_state: every cache, every step
                kc[i], vc[i] = kc[i].index_select(0, order), vc[i].index_select(0, order)
        return scores

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for B in a.batches:
        g = torch.Generator(device="cuda").manual_seed(B)
        enc = torch.randn(B, T, cfg.encoder_embed_dim, device="cuda", generator=g)
        lens = [T] * B
        with torch.no_grad():
            hyps = reader.generate_from_encoder(enc, lens)                      # warm-up: packs, captures
            assert reader.steps_run == steps + 1, reader.steps_run
            assert reader.sub_batches == 1, "the timed search must be ONE sub-batch of B clips: raise cache_bytes"
            for h in hyps:
                assert len(h) == beam and all(x["tokens"][-1] == EOS and len(x["tokens"]) == steps + 1 for x in h)
                assert [x["score"] for x in h] == sorted((x["score"] for x in h), reverse=True)
            torch_run(enc, 2)
            dev_ms, ref_ms = [], []
            for _ in range(a.repeats):                                          # alternate the two sides
                dev_ms.append(timed(lambda: reader.generate_from_encoder(enc, lens)) / (steps + 1))
                ref_ms.append(timed(lambda: torch_run(enc, steps + 1)) / (steps + 1))
            # launches of one step
            assert reader.sub_batches == 1
            S = reader._state(B, *reader.padded(T, steps), enc.device)["S"]                 # the state that was timed
            dec.start(S, [steps] * B)
            cnt = _Count()
            ops.set_profiler(cnt)
            dec.step(S, search)
            ops.set_profiler(None)
            torch.cuda.synchronize()
            dev_launches = len(cnt.records) + 1                                  # l2s_beam_advance is two kernels
            ref_launches = None
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    torch_run(enc, 3)
                    torch.cuda.synchronize()
                n = sum(e.count for e in prof.key_averages() if getattr(e, "device_time_total", 0) > 0 or getattr(e, "cuda_time_total", 0) > 0)
                ref_launches = round(n / 3)
            except Exception as e:                                              # the figure is optional, the timing is not
                ref_launches = None
                print(f"# torch.profiler unavailable: {e}", file=sys.stderr)
        md, mr = statistics.median(dev_ms), statistics.median(ref_ms)
        print(json.dumps({
            "B": B, "beam": beam, "V": V, "T_enc": T, "steps": steps + 1, "dtype": a.dtype,
            "device": {"ms_per_step": round(md, 4), "min": round(min(dev_ms), 4), "max": round(max(dev_ms), 4),
                       "tokens_per_s": round(B * beam * 1000.0 / md), "launches_per_step": dev_launches},
            "pytorch": {"ms_per_step": round(mr, 4), "min": round(min(ref_ms), 4), "max": round(max(ref_ms), 4),
                        "tokens_per_s": round(B * beam * 1000.0 / mr), "launches_per_step": ref_launches},
            "speedup": round(mr / md, 3)}), flush=True)


if __name__ == "__main__":
    main()
