"""The independent yardstick of the Whisper restatement (tests/_whisper_reference.py): transformers' WhisperFeatureExtractor and
WhisperForConditionalGeneration on the CPU in float64, fed with the seeded tiny weights through the package's rename table.
Imported only where transformers is (tests/test_whisper_cpu.py under importorskip, tools/make_whisper_golden.py)."""
import numpy as np
import torch

from tests import _whisper_reference as R


def hf_features(clip_i16):
    """WhisperFeatureExtractor's numpy path on one int16 clip -> [3000, 80].  Its result is float32 by construction."""
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor(feature_size=80, sampling_rate=16000, hop_length=160, chunk_length=30, n_fft=400)
    w = np.zeros(R.N_SAMPLES, np.float64)
    w[: len(clip_i16)] = clip_i16.astype(np.float64) / 32768.0
    return fe._np_extract_fbank_features(w[None], "cpu")[0].T.astype(np.float64)


def hf_model(sd, dims=R.TINY_DIMS):
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    from lip2speech_unit_amd.whisper import openai_to_hf
    cfg = WhisperConfig(vocab_size=dims["n_vocab"], num_mel_bins=dims["n_mels"], d_model=dims["n_audio_state"],
                        encoder_layers=dims["n_audio_layer"], decoder_layers=dims["n_text_layer"],
                        encoder_attention_heads=dims["n_audio_head"], decoder_attention_heads=dims["n_text_head"],
                        encoder_ffn_dim=4 * dims["n_audio_state"], decoder_ffn_dim=4 * dims["n_text_state"],
                        max_source_positions=dims["n_audio_ctx"], max_target_positions=dims["n_text_ctx"], activation_function="gelu",
                        pad_token_id=0, bos_token_id=1, eos_token_id=2, decoder_start_token_id=R.TINY_SOT[0], suppress_tokens=None,
                        begin_suppress_tokens=None, attn_implementation="eager")
    m = WhisperForConditionalGeneration(cfg).double().eval()
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in openai_to_hf(sd).items()}, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) <= {"proj_out.weight"}, res
    return m


@torch.no_grad()
def hf_encoder(m, feats):
    return m.model.encoder(torch.from_numpy(feats.T[None])).last_hidden_state[0].numpy()


@torch.no_grad()
def hf_logits(m, xa, tokens):
    from transformers.modeling_outputs import BaseModelOutput
    out = m(encoder_outputs=BaseModelOutput(last_hidden_state=torch.from_numpy(xa[None])),
            decoder_input_ids=torch.tensor([list(tokens)], dtype=torch.long), use_cache=False)
    return out.logits[0].numpy()


def hf_greedy(m, xa, steps):
    """The free-running greedy decode (no eot) on transformers' logits, with the tiny case's masks."""
    V = R.TINY_DIMS["n_vocab"]
    forbid = np.zeros(V, bool)
    forbid[list(R.TINY_SUPPRESS)] = True
    first = forbid.copy()
    first[list(R.TINY_BEGIN_SUPPRESS)] = True
    toks, ids = list(R.TINY_SOT), []
    for s in range(steps):
        t, _, _ = R.masked_argmax(hf_logits(m, xa, toks)[-1:], first if s == 0 else forbid)
        ids.append(int(t[0]))
        toks.append(int(t[0]))
    return ids
