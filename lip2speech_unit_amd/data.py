"""Input boundary of both stages (host side; file I/O only, no arithmetic beyond the reference's normalisation).

Stage 1 — `MultiTargetDataset` follows multi_target_lip2speech/dataset.py:37-257 on top of avhubert/hubert_dataset.py
(:242-245 transform, :317-321 load, :395-479 collate): tsv manifest + `.unt` labels, frames -> /255 -> CenterCrop(88) ->
(x-0.421)/0.165 -> [B,1,T,88,88] zero-padded to the longest clip with `padding_mask` (True = pad), `spk_emb`/`mel` sidecars.
Stage 2 — `parse_manifest`, `load_code_dict`, `code_to_sequence`, `MelCodeDataset` follow
multi_input_vocoder/dataset_multi_input.py:41-141,198-291 with segment_size = -1 (inference).

Video decode itself is outside the path: mp4 is read with OpenCV when it is importable, otherwise a
sibling `<clip>.npy` uint8 [T,H,W] array is used; nothing else is attempted.
"""
import os
import random
import wave
from typing import List

import numpy as np
import torch

from .plugin import DatasetBase


def load_video(path: str) -> np.ndarray:
    """avhubert/utils.py:13-30: grayscale uint8 frames [T,H,W]."""
    npy = os.path.splitext(path)[0] + ".npy"
    if os.path.exists(npy):
        return np.load(npy)
    try:
        import cv2  # type: ignore
    except ImportError as e:
        raise RuntimeError(f"cannot decode {path}: OpenCV is not installed and no {npy} sidecar exists") from e
    for attempt in range(3):
        cap = cv2.VideoCapture(path)
        frames = []
        while True:
            ret, frame = cap.read()
            if not ret:
                break
            frames.append(cv2.cvtColor(frame, cv2.COLOR_BGR2GRAY))
        if frames:
            return np.stack(frames)
    raise ValueError(f"Unable to load {path}")


def center_crop(frames: np.ndarray, size: int) -> np.ndarray:
    """avhubert/utils.py:75-95 (delta = int(round(w - tw) / 2.))."""
    t, h, w = frames.shape
    dw, dh = int(round(w - size) / 2.), int(round(h - size) / 2.)
    return frames[:, dh:dh + size, dw:dw + size]


def normalize_frames(frames_u8: np.ndarray, crop=88, mean=0.421, std=0.165) -> np.ndarray:
    """hubert_dataset.py:242-245: Normalize(0,255) -> CenterCrop -> Normalize(mean,std); returns fp32 [T,crop,crop]."""
    x = frames_u8.astype(np.float32) / 255.0
    x = center_crop(x, crop)
    return (x - mean) / std


class MultiTargetDataset(DatasetBase):
    """A FairseqDataset when fairseq is importable (plugin.py), so `task.get_batch_iterator` of the reference's decode loop
    (inference.py:164-179) can batch it: `num_tokens` / `size` / `ordered_indices` follow hubert_dataset.py:533-552."""

    def __init__(self, manifest_path, label_path=None, label_processor=None, pad=1, image_mean=0.421, image_std=0.165,
                 image_crop_size=88, text_label_path=None, mouth_cropper=None):
        """mouth_cropper (None: the video path is read with load_video): a callable video path -> gray uint8 [T, 96, 96] mouth
        ROIs, e.g. mouth_roi.VideoMouthCropper (raw frames + landmarks, cropped on the device)."""
        with open(manifest_path) as f:
            self.root = f.readline().strip()
            rows = [ln.rstrip("\n").split("\t") for ln in f if ln.strip()]
        # hubert_dataset.py load_audio_visual: (id, video path, audio path, n_frames, n_samples)
        self.names = [(r[1], r[2] + ":" + r[0]) for r in rows]
        self.ids = [r[0] for r in rows]
        self.sizes = [int(r[-2]) for r in rows]
        self.labels = None
        if label_path is not None and os.path.exists(label_path):
            with open(label_path) as f:
                self.labels = [ln.rstrip("\n") for ln in f]
            assert len(self.labels) == len(rows), "label file and manifest disagree"
        # text supervision (dataset.py:236-238): one line of space-separated piece ids per clip, tokenised beforehand
        self.text_labels = None
        if text_label_path is not None and os.path.exists(text_label_path):
            with open(text_label_path) as f:
                self.text_labels = [np.asarray([int(x) for x in ln.split()], dtype=np.int64) for ln in f.read().splitlines()]
            assert len(self.text_labels) == len(rows), "text label file and manifest disagree"
        self.label_processor = label_processor
        self.label_processors = [label_processor]
        self.pad = pad
        self.mean, self.std, self.crop = image_mean, image_std, image_crop_size
        self.mouth_cropper = mouth_cropper

    def __len__(self):
        return len(self.ids)

    def num_tokens(self, index):
        return self.sizes[index]

    def size(self, index):
        return self.sizes[index]

    def ordered_indices(self):
        # shuffle=False at inference (inference.py:179): longest first, ties in manifest order
        return np.lexsort((np.arange(len(self)), self.sizes))[::-1]

    def _sidecar(self, video_fn, kind):
        return os.path.join(self.root, video_fn).replace("/video/", f"/{kind}/")[:-4] + ".npy"  # dataset.py:197-212

    def __getitem__(self, index):
        video_fn = self.names[index][0]
        path = os.path.join(self.root, video_fn)
        frames = load_video(path) if self.mouth_cropper is None else np.asarray(self.mouth_cropper(path))
        feats = normalize_frames(frames, self.crop, self.mean, self.std)
        sample = {"id": index, "fid": self.ids[index], "names": self.names[index],
                  "video_source": torch.from_numpy(np.ascontiguousarray(feats)), "audio_source": None}
        if self.labels is not None and self.label_processor is not None:
            sample["label_list"] = [self.label_processor(self.labels[index])]
        for kind in ("mel", "spk_emb"):
            p = self._sidecar(video_fn, kind)
            if not os.path.exists(p):
                raise FileNotFoundError(f"{p} does not exist")
            sample[kind] = torch.from_numpy(np.load(p).astype(np.float32))
        if self.text_labels is not None:
            sample["text_labels"] = torch.from_numpy(self.text_labels[index])
        return sample

    def collater(self, samples: List[dict]):
        """hubert_dataset.py:395-479 + dataset.py:242-257 (pad_audio=True: pad to the longest clip)."""
        B = len(samples)
        T = max(s["video_source"].shape[0] for s in samples)
        H, W = samples[0]["video_source"].shape[1:]
        video = torch.zeros(B, 1, T, H, W)
        padding_mask = torch.zeros(B, T, dtype=torch.bool)
        for i, s in enumerate(samples):
            n = s["video_source"].shape[0]
            video[i, 0, :n] = s["video_source"]
            padding_mask[i, n:] = True
        batch = {"id": torch.tensor([s["id"] for s in samples]), "utt_id": [s["fid"] for s in samples],
                 "names": [s["names"] for s in samples],
                 "net_input": {"source": {"audio": None, "video": video}, "padding_mask": padding_mask,
                               "spk_emb": torch.stack([s["spk_emb"] for s in samples])},
                 "input_lengths": torch.tensor([s["video_source"].shape[0] for s in samples], dtype=torch.int32)}
        if "label_list" in samples[0]:
            labs = [s["label_list"][0] for s in samples]
            L = max(len(x) for x in labs)
            tgt = torch.full((B, L), self.pad, dtype=torch.long)
            for i, x in enumerate(labs):
                tgt[i, : len(x)] = x
            batch["target"] = tgt
            batch["target_lengths"] = torch.tensor([len(x) for x in labs])
            batch["ntokens"] = int(sum(len(x) for x in labs))
        else:
            batch["target"] = None
        mlen = max(len(s["mel"]) for s in samples)
        batch["mel"] = torch.stack([torch.nn.functional.pad(s["mel"], [0, 0, 0, mlen - len(s["mel"])]) for s in samples])
        if "text_labels" in samples[0]:                                   # dataset.py:250-255: 1-D, no padding
            batch["text_labels"] = torch.cat([s["text_labels"] for s in samples]).int()
            batch["text_labels_lengths"] = torch.tensor([s["text_labels"].shape[0] for s in samples], dtype=torch.int32)
        return batch


# ---- stage 2 -----------------------------------------------------------------------------------------------------
def repeat_text_labels(labels):
    """dataset_multi_input.py:23-38 `repeat`: CTC blanks (0) and label changes forward-filled from the first label."""
    out, cur = [labels[0]], labels[0]
    for x in labels[1:]:
        if x != 0 and x != cur:
            cur = x
        out.append(cur)
    return out


def parse_manifest(manifest_path, max_keep=None, min_keep=None):
    """dataset_multi_input.py:41-110: returns (audio_files, mel_files, codes), plus t_labels (lists of int) when
    TEXT_SUPERVISION=1 and the label file <manifest>.txt exists: one line per KEPT utterance (the reference reads a line only
    for rows it keeps), forward-filled under REPEAT_TEXT_LABELS=1."""
    audio_files, mels, codes, t_labels = [], [], [], []
    code_path = os.path.splitext(manifest_path)[0] + ".unt"
    t_path = os.path.splitext(manifest_path)[0] + ".txt"
    text = bool(int(os.environ.get("TEXT_SUPERVISION", 0))) and os.path.exists(t_path)
    rep = text and bool(int(os.environ.get("REPEAT_TEXT_LABELS", 0)))
    f_t = open(t_path) if text else None
    with open(manifest_path) as f, open(code_path) as f_c:
        root = f.readline().strip()
        for line, line_code in zip(f, f_c):
            items = line.strip().split("\t")
            code = line_code.strip().split("|")[-1]
            sz = int(items[-2])
            diff = len(code.split()) - sz * 2
            assert -2 <= diff <= 2, "code length != video length * 2"
            if (min_keep is not None and sz < min_keep) or (max_keep is not None and sz > max_keep):
                continue
            audio_path = os.path.join(root, items[2])
            audio_files.append(audio_path)
            mels.append(audio_path.replace("/audio/", "/mel/")[:-4] + ".npy")
            codes.append(code)
            if text:
                t = [int(x) for x in f_t.readline().strip().split(" ")]
                t_labels.append(repeat_text_labels(t) if rep else t)
    if not text:
        return audio_files, mels, codes
    f_t.close()
    return audio_files, mels, codes, t_labels


def load_code_dict(path):
    """dataset_multi_input.py:118-125: symbol -> line index (raw unit id, NOT the +4 fairseq token id)."""
    with open(path) as f:
        syms = [line.rstrip().rsplit(" ", 1)[0] for line in f]
    d = {c: i for i, c in enumerate(syms)}
    assert set(d.values()) == set(range(len(d)))
    return d


def code_to_sequence(code, code_dict, collapse_code=False):
    """dataset_multi_input.py:128-141."""
    if collapse_code:
        seq, prev = [], None
        for c in code:
            if c in code_dict and c != prev:
                seq.append(code_dict[c])
                prev = c
        return seq
    return [code_dict[c] for c in code if c in code_dict]


def audio_num_samples(path, pad=None):
    """The reference reads the wav only for its length (dataset_multi_input.py:201-213,222-239)."""
    with wave.open(path, "rb") as w:
        n = w.getnframes()
    if pad:
        n += pad - (n % pad)
    return n


class MelCodeDataset:
    def __init__(self, file_list, code_hop_size=320, mel_hop_size=160, code_dict_path=None, pad=None, mel_from_audio=False,
                 stft=None, segment_size=None, seed=1234, load_audio=False, sampling_rate=16000, spk_embedder=None):
        """spk_embedder (None: spk_emb/<name>.npy is read): a callable wav path -> float32 (256,), e.g.
        speaker_encoder.SpeakerEncoder.embed_file - the embedding is computed from the clip's audio and spk_emb/ is not touched.

        mel_from_audio: the mel/ directory is not touched - the wav is read, zero-extended to the padded length and analysed
        on the device (audio.TacotronSTFT, or `stft`: anything with its mel_rows) before the same trimming rule applies.

        segment_size (None: today's inference items, audio not read unless load_audio): the training / validation items of
        dataset_multi_input.py:198-291.  The wav is read as int16 (another sampling rate is refused: there is no resampler here),
        taken as value / 32768 in float64, divided by its peak and multiplied by 0.95 (:211-212, librosa.util.normalize on a 1-d
        signal), trimmed with code and mel (:219-241), and while it is shorter than the segment audio, code and mel are doubled
        (:249-255).  Then _sample_interval (speech-resynthesis/dataset.py:199-219) cuts the same stretch out of all three: with
        the sequences audio / code / mel the common step is code_hop_size samples and start = randint(0, L - segment_size //
        code_hop_size) code frames, ONE draw per __getitem__ call - so reading the items once in index order reproduces the
        reference's draws.  They come from a random.Random(seed) owned by this object; the reference seeds the module-level
        generator in its constructor (:154), an instance keeps other users of `random` out of the sequence.  segment_size <= 0:
        the whole clip, start 0, no draw.  Items are (feats, audio float32 [segment], filename, None); `starts[index]` keeps the
        start of the last read in code frames.  Note that `split=False` at train.py:117 has no effect in the reference -
        __getitem__ never reads it - so its validation does run on random 8960-sample segments, and so does this."""
        self.audio_files, self.mel_files, self.codes = file_list[:3]
        self.mel_from_audio, self.stft = mel_from_audio, stft
        self.t_labels = file_list[3] if len(file_list) > 3 else None   # text supervision (dataset_multi_input.py:225-239)
        self.code_hop_size, self.mel_hop_size, self.pad = code_hop_size, mel_hop_size, pad
        self.segment_size, self.load_audio, self.sampling_rate = segment_size, load_audio or segment_size is not None, sampling_rate
        self.rng, self.starts = random.Random(seed), {}
        self.code_dict = load_code_dict(code_dict_path)
        self.speaker_emb_files = [f.replace("/audio/", "/spk_emb/")[:-4] + ".npy" for f in self.audio_files]
        self.spk_embedder = spk_embedder

    def __len__(self):
        return len(self.audio_files)

    def analyse(self, filename, n_audio):
        """[T, n_mel] log-mel of the wav, zero-extended to n_audio samples (what --pad does to the length)."""
        import torch
        from . import audio
        stft = self.stft if self.stft is not None else audio.default_stft()
        pcm = audio.read_wav_s16(filename)
        wav = np.zeros(n_audio, np.int16)
        wav[: pcm.shape[0]] = pcm[:n_audio]
        wav = torch.from_numpy(wav).unsqueeze(0)
        if self.stft is None:
            wav = wav.cuda()
        return np.asarray(stft.mel_rows(wav)[0].cpu())

    def __getitem__(self, index):
        """dataset_multi_input.py:198-291 with segment_size=-1: (feats{code,mel,spkr[,t_label]}, None, filename, None)."""
        filename = self.audio_files[index]
        n_audio = audio_num_samples(filename, self.pad)
        code = np.array(code_to_sequence(self.codes[index].split(), self.code_dict))
        code_length = min(n_audio // self.code_hop_size, code.shape[0])
        code = code[:code_length]
        t_label = None
        if self.t_labels is not None:
            t_label = np.asarray(self.t_labels[index], dtype=np.int64)[:code_length]
            assert t_label.shape[0] == code.shape[0], f"{filename}: {t_label.shape[0]} != {code.shape[0]}"
        mel = self.analyse(filename, n_audio) if self.mel_from_audio else np.load(self.mel_files[index])
        mel_length = min(n_audio // self.mel_hop_size, mel.shape[0])
        mel = mel[:mel_length]
        cut = min(mel_length * self.mel_hop_size, code_length * self.code_hop_size)
        mel = mel[: cut // self.mel_hop_size]
        code = code[: cut // self.code_hop_size]
        assert cut // self.code_hop_size == code.shape[0], "Code audio mismatch"
        assert cut // self.mel_hop_size == mel.shape[0], "Mel audio mismatch"
        mel = mel.transpose(1, 0)
        wav = None
        if self.load_audio:
            wav, code, mel, t_label = self._segment(index, filename, n_audio, cut, code, mel,
                                                    None if t_label is None else t_label[: cut // self.code_hop_size])
        feats = {"code": code.astype(np.int64), "mel": np.ascontiguousarray(mel).astype(np.float32),
                 "spkr": (np.load(self.speaker_emb_files[index]) if self.spk_embedder is None
                          else np.asarray(self.spk_embedder(filename))).astype(np.float32)}
        if t_label is not None:
            feats["t_label"] = t_label[: cut // self.code_hop_size] if wav is None else t_label
        return feats, wav, str(filename), None

    def _segment(self, index, filename, n_audio, cut, code, mel, t_label):
        """The audio side of dataset_multi_input.py:201-273 (see __init__): returns (audio float32, code, mel [80, .], t_label)."""
        from . import audio as _audio
        pcm = _audio.read_wav_s16(filename, self.sampling_rate)
        x = np.zeros(n_audio, np.float64)                                     # :208-210 --pad zero-extends
        x[: pcm.shape[0]] = pcm
        x = x / 32768.0
        peak = np.abs(x).max()
        x = (x / peak if peak > 0 else x) * 0.95                              # :211-212
        x = x[:cut]                                                           # :239
        seg = self.segment_size if self.segment_size is not None else -1
        while x.shape[0] < seg:                                               # :249-255
            x, code, mel = np.hstack([x, x]), np.hstack([code, code]), np.hstack([mel, mel])
            if t_label is not None:
                t_label = np.hstack([t_label, t_label])
        x = x.astype(np.float32)                                              # :257 torch.FloatTensor
        seqs = [x, code, mel] + ([t_label] if t_label is not None else [])
        N = max(v.shape[-1] for v in seqs)                                    # speech-resynthesis/dataset.py:199-219
        seq_len = seg if seg > 0 else N
        hops = [N // v.shape[-1] for v in seqs]
        lcm = int(np.lcm.reduce(hops))
        start = self.rng.randint(0, N // lcm - seq_len // lcm) if seg > 0 else 0
        self.starts[index] = start
        out = [v[..., start * (lcm // hp): (start + seq_len // lcm) * (lcm // hp)] for v, hp in zip(seqs, hops)]
        return out[0], out[1], out[2], (out[3] if t_label is not None else None)
