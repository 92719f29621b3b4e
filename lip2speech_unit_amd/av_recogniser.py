"""Audio-visual speech recognition on gfx950: the AV-HuBERT seq2seq model of the reference tree decoded from audio, video or both,
as `avhubert/infer_s2s.py` decodes it with `override.modalities` (the `conf/av-finetune/*.yaml` models, `modalities:
["video", "audio"]`).

  audio rows  audio.LogFbank: `logfbank(wav, samplerate=16000)`, the stacker, the alignment to the video's frame count and
              F.layer_norm of hubert_dataset.py:299-315,370-372 in one launch (csrc/logfbank.hip), in the model's 16-bit type
  encoder     hubert.AVHubertModel.extract_av_rows: the two projections into the halves of one buffer (or added), layer_norm,
              post_extract_proj, the transformer encoder
  search      lip_reader.LipReader.generate_from_encoder, unchanged

Video alone returns exactly what LipReader returns.  Out of scope: noise mixing (`noise_prob`), training-time modality dropout."""
import torch

from . import ops
from .audio import LogFbank, logfbank_rows
from .lip_reader import LipReader, read_seq2seq_checkpoint
from .plugin import cfg_get

MODALITIES = ("audio", "video")


def modality_set(mods, what="modalities"):
    """['video', 'audio'] in any order -> the sorted tuple; anything but a non-empty subset of {audio, video} is a ValueError."""
    names = tuple(sorted({str(m) for m in mods}))
    if not names or any(m not in MODALITIES for m in names):
        raise ValueError(f"{what} = {list(mods)}: a non-empty subset of {list(MODALITIES)}")
    return names


def _flag(v, default):
    if v is None:
        return default
    return v.strip().lower() in ("true", "1") if isinstance(v, str) else bool(v)


def load_speech_recogniser(path, dtype=ops.F16, modalities=None):
    """A fine-tuned AV-HuBERT seq2seq checkpoint (the layout load_lip_reader reads) of any modality set -> AVHubertSeq2Seq in eval
    mode with `modalities` (the argument, else cfg.task.modalities, else video), `stack_order_audio` and `normalize` (cfg.task;
    4 and true when absent) set on it."""
    seen = []

    def accept(mods):
        seen.append(modality_set(mods, "task.modalities") if mods is not None else ("video",))
    model, task, absent = read_seq2seq_checkpoint(path, dtype, accept)
    mods = modality_set(modalities) if modalities is not None else seen[0]
    stack = int(cfg_get(task, "stack_order_audio", 4)) if task is not None else 4
    normalize = _flag(cfg_get(task, "normalize", None) if task is not None else None, True)
    if "audio" in mods:
        lacking = [k for k in absent if "feature_extractor_audio" in k]
        if lacking:
            raise ValueError(f"{path}: the audio modality needs {lacking}, which the checkpoint does not hold")
        feat = model.encoder.w2v_model.cfg.audio_feat_dim
        if feat != 26 * stack:
            raise ValueError(f"{path}: audio_feat_dim = {feat} but stack_order_audio = {stack} gives rows of {26 * stack}")
    model.modalities, model.stack_order_audio, model.normalize = mods, stack, normalize
    return model


class SpeechRecogniser(LipReader):
    """LipReader over audio and / or video.  `generate(video, wav, n_samples, padding_mask)`: video [B, 1, T, 88, 88] or None; wav
    a device tensor [B, S], int16 PCM or float at int16 scale, 16 kHz, padded, or None; n_samples the clips' sample counts (host
    sequence; None = S); padding_mask bool [B, T] or None.  A clip has the video's frame count of rows when video is given (the
    audio rows are padded or trimmed to it), else logfbank_rows(n, stack).  The streams the model's `modalities` leave out are
    dropped, as the reference's dataset does not load them."""

    def __init__(self, model, dictionary=None, config=None, modalities=None, **kw):
        """modalities: default the model's (load_speech_recogniser sets them; a model built by hand is video only).  The features'
        `stack_order_audio` and `normalize` are the model's too, 4 and true on a model built by hand."""
        super().__init__(model, dictionary, config, **kw)
        self.modalities = modality_set(modalities if modalities is not None else getattr(model, "modalities", ("video",)))
        self.features = None
        if "audio" in self.modalities:
            self.features = LogFbank(getattr(model, "stack_order_audio", 4), getattr(model, "normalize", True))

    def audio_rows(self, wav, n_samples=None, n_rows=None, T=None):
        """The audio sub-model's input: rows [B, T, 26 * stack] in the model's 16-bit type and the per-clip row counts."""
        B, S = wav.shape
        ns = [int(v) for v in (n_samples if n_samples is not None else [S] * B)]
        if len(ns) != B or any(n <= 0 or n > S for n in ns):
            raise ValueError(f"n_samples: every clip needs 0 < n <= {S} samples, got {ns}")
        counts = [int(v) for v in n_rows] if n_rows is not None else [logfbank_rows(n, self.features.stack) for n in ns]
        T = max(counts) if T is None else T
        rows = self.features.rows(wav, ns, counts, T_rows=T, dtype=ops.torch_dtype(self.model.dtype))
        return rows, counts

    def encode(self, video=None, wav=None, n_samples=None, padding_mask=None):
        """-> (fp32 rows [B * T, d_enc], lens int32 [B], B, T) of hubert.AVHubertModel.extract_av_rows."""
        if isinstance(video, dict):
            raise ValueError("pass video and wav separately; the reference's `source` dict carries features, not waveforms")
        video = video if "video" in self.modalities else None
        wav = wav if "audio" in self.modalities else None
        if video is None and wav is None:
            raise ValueError(f"modalities = {list(self.modalities)}: none of them was given")
        w2v = self.model.encoder.w2v_model
        if wav is None:
            return w2v.extract_av_rows(video=video, padding_mask=padding_mask)
        if video is not None:
            B, T = video.shape[0], video.shape[2]
            frames = [T] * B if padding_mask is None else (T - padding_mask.to(torch.int64).sum(1)).cpu().tolist()
            rows, _ = self.audio_rows(wav, n_samples, frames, T)
            return w2v.extract_av_rows(audio=rows, video=video, padding_mask=padding_mask)
        rows, counts = self.audio_rows(wav, n_samples)
        T = rows.shape[1]
        mask = None
        if min(counts) < T:
            mask = (torch.arange(T)[None, :] >= torch.tensor(counts)[:, None]).to(wav.device)
        return w2v.extract_av_rows(audio=rows, padding_mask=mask)

    @torch.no_grad()
    def generate(self, video=None, wav=None, n_samples=None, padding_mask=None):
        rows, lens, B, T = self.encode(video, wav, n_samples, padding_mask)
        return self.generate_from_encoder(rows.view(B, T, -1), lens.cpu().tolist())

    def transcribe(self, video=None, wav=None, n_samples=None, padding_mask=None):
        if self.dictionary is None:
            raise ValueError("SpeechRecogniser.transcribe needs a dictionary; generate() does not")
        return [self.dictionary.string(h[0]["tokens"]) if h else "" for h in self.generate(video, wav, n_samples, padding_mask)]
