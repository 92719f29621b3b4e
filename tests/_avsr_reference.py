"""float64 reference of the two-stream AVHubertModel.extract_finetune (avhubert/hubert.py:694-745): oracle.avhubert's `_lin`, `_ln`
and `transformer_encoder` plus the audio branch of :703-727 - the audio sub-model is its projection alone (SubModel with no
resnet, :317-332), an absent stream is zeros of the encoder's width, 'concat' puts audio left of video, 'add' sums them.  The
audio rows come from tests/_logfbank_reference.py (float64, aligned to the video's frame count)."""
import numpy as np
import torch

from oracle import avhubert as oa
from oracle import frontend

from . import _logfbank_reference as LR


def audio_rows(clips, n_rows, T, stack=4, normalize=True):
    """float64 [B, T, 26 * stack]: each clip's rows aligned to n_rows[b] (None: its own count), zeros up to T."""
    out = np.zeros((len(clips), T, LR.NFILT * stack))
    for b, c in enumerate(clips):
        r = LR.audio_rows(c, stack, None if n_rows is None else n_rows[b], normalize)
        out[b, :len(r)] = r
    return torch.from_numpy(out)


def extract_finetune(sd, audio, video, padding_mask, fuse="concat", layers=1, heads=16, p="encoder.w2v_model"):
    """sd: state dict (any float type; used in float64).  audio: float64 [B, T, F] or None; video: [B, 1, T, 88, 88] or None;
    padding_mask: bool [B, T] or None -> x float64 [B, T, C]."""
    sd = {k: v.detach().cpu().double() for k, v in sd.items() if k.startswith(p + ".")}
    fa = fv = None
    if video is not None:
        fsd = {k[len(p) + len(".feature_extractor_video.resnet."):]: v for k, v in sd.items()
               if k.startswith(p + ".feature_extractor_video.resnet.")}
        feat = frontend.res_encoder(fsd, video.double())                                    # [B, 512, T]
        fv = oa._lin(sd, p + ".feature_extractor_video.proj", feat.transpose(1, 2))        # [B, T, C]  :327
    if audio is not None:
        fa = oa._lin(sd, p + ".feature_extractor_audio.proj", audio.double())               # :327, no resnet
    if fa is None:
        fa = torch.zeros_like(fv)                                                            # :708
    if fv is None:
        fv = torch.zeros_like(fa)                                                            # :705
    feats = torch.cat([fa, fv], dim=2) if fuse == "concat" else fa + fv                      # :712-715
    feats = oa._ln(sd, p + ".layer_norm", feats)                                             # :720
    x = oa._lin(sd, p + ".post_extract_proj", feats)                                         # :727
    return oa.transformer_encoder(sd, p + ".encoder", x, padding_mask, layers, heads)        # :739
