"""Device-resident lip -> units -> waveform pipeline (no host synchronisation, hipGraph-capturable).

Strings the reference's two stages together without the file round trip between them
(multi_target_lip2speech/inference.py:267-274 -> create_dataset.py:366-428 -> multi_input_vocoder/dataset_multi_input.py:
198-291): predicted unit tokens t -> vocoder code t-4 (dict.unt.txt lists units 0..199 in order, fairseq prepends 4
specials), predicted mel [4*src_len, 80] -> vocoder mel [80, 4*src_len]; both already have code_len*320 == mel_len*160 so
the reference's trimming rule is the identity here.
"""
import os
from typing import Optional

import torch

from . import ops
from .packing import state_epoch


class GraphCache:
    """hipGraph replay for a device-only callable: captured once per input signature (shapes / dtypes), replayed afterwards.
    An eager batch costs ~900 launches x ~10 us of host time - more than the GPU needs for a small batch - so the CLIs and
    servers route their device part through this; `bench.py` captures its fixed shape itself.  Inputs are copied into the
    capture's static tensors; the returned tensors are the capture's static outputs (valid until the next call with the
    same signature).  At most `max_entries` captures are kept (least recently used dropped: its private memory pool goes with it).
    A capture holds raw pointers into the packed weights `fn` reads: `state`, when given, is a callable whose value changes
    whenever those are rebuilt (`packing.state_epoch` of the models), and a changed value drops every capture."""

    def __init__(self, fn, max_entries: int = 8, state=None):
        self.fn, self.max_entries, self.state = fn, max_entries, state
        self.entries = {}
        self.captures = 0
        self._state_seen = None

    def _drop_if_state_changed(self):
        s = self.state() if self.state is not None else None
        if s != self._state_seen:
            self.entries.clear()
            self._state_seen = s

    def __call__(self, *tensors):
        self._drop_if_state_changed()
        key = tuple((tuple(t.shape), t.dtype) if t is not None else None for t in tensors)
        e = self.entries.get(key)
        if e is None:
            static_in = [t.clone() if t is not None else None for t in tensors]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):            # warm-up: allocations, packed weights, cached position tables
                self.fn(*static_in)
                self.fn(*static_in)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self._drop_if_state_changed()            # the warm-up packed: that is the state the capture below belongs to
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = self.fn(*static_in)
            if len(self.entries) >= self.max_entries:
                self.entries.pop(next(iter(self.entries)))
            e = self.entries[key] = (g, static_in, out)
            self.captures += 1
        else:
            self.entries[key] = self.entries.pop(key)      # most recently used last: eviction above drops the LRU entry
            for dst, src in zip(e[1], tensors):
                if dst is not None:
                    dst.copy_(src, non_blocking=True)
        e[0].replay()
        return e[2]


def text_decode(conformer, y16, lens, B, T2, beam_search=False):
    """CTC text head of a text-supervised conformer on its y16 rows, decoded on the device: {"text_logits", "text"} and under
    beam_search {"text_beams", "text_lens", "text_scores"} (ops.ctc_decode)."""
    tl = conformer.text_rows(y16)
    Vt = conformer.text_classes
    d = ops.ctc_decode(tl, B=B, L=T2, V=Vt, ldl=tl.shape[1], lens=lens, len_mul=2, beam=30 if beam_search else 0, K=40, nbest=3)
    d["text_logits"] = tl.view(B, T2, -1)
    return d


class LipToSpeechPipeline:
    def __init__(self, model, vocoder, temperature: float = 1.0, len_penalty: float = 1.0):
        self.model, self.vocoder = model, vocoder
        self.temperature, self.len_penalty = temperature, len_penalty
        self._shared_ready = set()
        # text-supervised checkpoints: CTC prefix beam search instead of the framewise argmax (sequence_generator.py:20-38)
        self.ctc_beam = int(os.environ.get("CTC_BS_DECODING", "0")) != 0
        # text-supervised vocoders: its label file forward-filled (dataset_multi_input.py:23-38, REPEAT_TEXT_LABELS=1)
        self.repeat_text = int(os.environ.get("REPEAT_TEXT_LABELS", "0")) != 0

    def _shared_state_key(self, dev, T):
        """Identity of the lazily built state sub-batches share: device, frames per clip and the packed-state epoch of the two
        models (it moves whenever a module under them packs or drops its weights, and never returns to an earlier value)."""
        return (str(dev), int(T), state_epoch(self.model, self.vocoder))

    @torch.no_grad()
    def stage1_device(self, video, padding_mask, spk_emb):
        """Returns dict of device tensors: tokens int32 [B,2T+1], lprobs, score, mel fp32 [B,4T,80], logits, lens.  With a text
        head (TEXT_SUPERVISION=1) also text int32 [B,2T] (framewise CTC argmax, 0 past a clip's length) and text_logits
        fp32 [B,2T,Vp]; under CTC_BS_DECODING=1 text_beams int32 [B,3,2T], text_lens [B,3], text_scores [B,3] (the top 3 of
        a 30-wide prefix beam search over the 40 most probable classes per frame)."""
        m = self.model
        enc_mod = m.encoder.w2v_model if hasattr(m.encoder, "w2v_model") else m.encoder   # AV-HuBERT / Auto-AVSR encoder
        enc, lens, B, T = enc_mod.extract_rows(video, padding_mask)
        dt = m.conformer.dtype
        src16 = torch.empty(B * 2 * T, enc.shape[1], device=enc.device, dtype=ops.torch_dtype(dt))
        ops.repeat2_cast(enc, src16, B, T, enc.shape[1], dt)
        logits, mel, y16 = m.conformer.forward_rows(src16, lens, B, 2 * T, spk_emb, len_mul=2)
        T2, V = 2 * T, logits.shape[1]
        tokens = torch.empty(B, T2 + 1, device=enc.device, dtype=torch.int32)
        lprobs = torch.empty(B, T2 + 1, device=enc.device, dtype=torch.float32)
        score = torch.empty(B, device=enc.device, dtype=torch.float32)
        ops.greedy_decode(logits, tokens, lprobs, score, B=B, T2=T2, V=V, lens=lens, len_mul=2,
                          temperature=self.temperature, lenpen=self.len_penalty)
        out = {"tokens": tokens, "lprobs": lprobs, "score": score, "mel": mel.view(B, 2 * T2, -1),
               "logits": logits.view(B, T2, V), "lens": lens, "encoder_out": enc.view(B, T, -1)}
        if getattr(m.conformer, "text_classifier", None) is not None:
            out.update(text_decode(m.conformer, y16, lens, B, T2, self.ctc_beam))
        return out

    @torch.no_grad()
    def stage2_device(self, s1, spk_emb):
        """units/mel of stage 1 -> (wav fp32 [B, 640*T], pcm int16).  Rows past each clip's length come out as zero."""
        # token -> unit id, mel [B,4T,80] -> the vocoder's channels-last concat columns, lens -> row masks: all inside the
        # vocoder's own launches (no torch arithmetic / layout kernels between the stages)
        return self.vocoder.forward_tokens_rows(s1["tokens"], s1["mel"], spk_emb, s1["lens"], t_rows=self.text_rows(s1))

    def text_rows(self, s1):
        """The frame labels a text-supervised vocoder reads: stage 1's FRAMEWISE argmax labels whatever the decode mode
        (create_dataset.py:402-425 copies pred_text's first line, which only has the code's length for greedy output),
        forward-filled under REPEAT_TEXT_LABELS=1.  None for a vocoder without the text branch."""
        if not getattr(self.vocoder, "text_supervision", False):
            return None
        if "text" not in s1:
            raise ValueError("the vocoder is text-supervised but the stage-1 model has no text head (TEXT_SUPERVISION)")
        t = s1["text"]
        if self.repeat_text:
            B, L = t.shape
            filled = torch.empty_like(t)
            ops.ctc_repeat_labels(t, filled, B=B, L=L, lens=s1["lens"], len_mul=2)
            t = filled
        return t

    @torch.no_grad()
    def forward_device(self, video, padding_mask, spk_emb):
        s1 = self.stage1_device(video, padding_mask, spk_emb)
        wav, pcm = self.stage2_device(s1, spk_emb)
        s1["wav"], s1["pcm"] = wav, pcm
        return s1

    @torch.no_grad()
    def forward_device_u8(self, frames_u8, padding_mask, spk_emb, crop: int = 88, mean: float = 0.421, std: float = 0.165,
                          fused: Optional[bool] = None):
        """On-device input pipeline: uint8 grayscale frames [B,T,Hin,Win] straight from the decoder ->
        centre crop + (x/255 - mean)/std (hubert_dataset.py:242-245, utils.py:56-95) applied inside the stem kernel's
        frame fetch, then the normal path: a quarter of the fp32 frames' PCIe bytes, no CPU numpy pass, and the
        normalised frames are never written to HBM.  fused=False keeps the separate l2s_preprocess_frames launch (same
        bits; the A/B and the parity test use it)."""
        B, T, Hin, Win = frames_u8.shape
        if fused is None:
            fused = os.environ.get("L2S_STEM_U8", "1") != "0"
        enc_mod = self.model.encoder.w2v_model if hasattr(self.model.encoder, "w2v_model") else self.model.encoder
        resnet = getattr(getattr(enc_mod, "feature_extractor_video", None), "resnet", None)   # AV-HuBERT's ResEncoder
        if fused and crop == 88 and resnet is not None:
            resnet.u8_transform = (crop, mean, std)
            return self.forward_device(frames_u8.contiguous(), padding_mask, spk_emb)
        dt = resnet.dtype if resnet is not None else self.model.conformer.dtype
        x = torch.empty(B, 1, T, crop, crop, device=frames_u8.device, dtype=ops.torch_dtype(dt))
        ops.preprocess_frames(frames_u8.contiguous(), x, B=B, T=T, Hin=Hin, Win=Win, crop=crop, mean=mean, std=std, dtype=dt)
        return self.forward_device(x, padding_mask, spk_emb)

    @torch.no_grad()
    def forward_device_u8_streams(self, frames_u8, padding_mask, spk_emb, streams: int = 2, **kw):
        """The batch as `streams` independent sub-batches (clips are independent: same results), each on its own HIP
        stream, forked from and joined to the caller's stream - capturable into ONE hipGraph.  Every kernel of the path ends
        with a tail (the last round of tiles, the epilogue's store burst) in which part of the chip idles; a second stream
        fills it with the other sub-batch's next kernel.  Measured on one box (`tools/dual_stream_exp.py`): 640 clips as
        one batch 230.5 ms, as 2 x 320 on two streams 222.9 ms; 160 clips 59.9 ms -> 55.7 ms per 160 clips.
        Returns the sub-batches' outputs concatenated along the clip axis (tokens, lens, score, mel, wav, pcm)."""
        B = frames_u8.shape[0]
        if streams <= 1 or B < streams:
            return self.forward_device_u8(frames_u8, padding_mask, spk_emb, **kw)
        if getattr(self, "_side_streams", None) is None or len(self._side_streams) != streams:
            self._side_streams = [torch.cuda.Stream(device=frames_u8.device) for _ in range(streams)]
        cur = torch.cuda.current_stream()
        # State every sub-batch shares is built lazily by the first forward that needs it: packed weights (per module and
        # device) and the conformer's projected position table (per T).  Built inside sub-batch 0 it would be enqueued on
        # side stream 0 only, and the other streams would read it with no dependency.  So the first time a (device, T, set
        # of packed weights) is seen, one clip runs on the CALLER's stream, which every side stream waits on below.
        key = self._shared_state_key(frames_u8.device, frames_u8.shape[1])
        if key not in self._shared_ready:
            pm1 = None if padding_mask is None else padding_mask[:1]
            self.forward_device_u8(frames_u8[:1], pm1, spk_emb[:1], **kw)
            self._shared_ready.add(self._shared_state_key(frames_u8.device, frames_u8.shape[1]))
        bounds = [B * i // streams for i in range(streams + 1)]
        outs = []
        for i, st in enumerate(self._side_streams):
            lo, hi = bounds[i], bounds[i + 1]
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                pm = None if padding_mask is None else padding_mask[lo:hi]
                outs.append(self.forward_device_u8(frames_u8[lo:hi], pm, spk_emb[lo:hi], **kw))
        for st in self._side_streams:
            cur.wait_stream(st)
        keys = ("tokens", "lens", "score", "mel", "wav", "pcm") + tuple(k for k in ("text", "text_beams", "text_lens", "text_scores")
                                                                       if k in outs[0])
        return {k: torch.cat([o[k] for o in outs]) for k in keys}

    @torch.no_grad()
    def __call__(self, video, padding_mask, spk_emb):
        """Host-facing call: list of (unit ids np.int64 [L], mel np [2L,80], pcm np.int16 [320L]) per clip."""
        out = self.forward_device(video, padding_mask, spk_emb)
        lens = out["lens"].tolist()
        toks, mel, pcm = out["tokens"].cpu().numpy(), out["mel"].cpu().numpy(), out["pcm"].cpu().numpy()
        res = []
        for b, n in enumerate(lens):
            L = 2 * n
            res.append((toks[b, :L].astype("int64") - 4, mel[b, : 2 * L], pcm[b, : 320 * L]))
        return res
