"""Writes tests/golden/whisper_tiny.npz: small recorded results of transformers (WhisperFeatureExtractor, and
WhisperForConditionalGeneration in float64 on the CPU) for the seeded tiny cases of tests/_whisper_reference.py - every 25th
feature frame of clip 0, the encoder output rows 0, 700 and 1499 of every clip, the teacher-forced logit rows of every clip and the
free-running greedy ids.  No weights: they are regenerated from the seed.  Needs transformers; run from the repository root:

    python tools/make_whisper_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _whisper_hf as HF  # noqa: E402
from tests import _whisper_reference as R  # noqa: E402

FEATURE_STRIDE, ENC_ROWS = 25, (0, 700, 1499)


def main():
    case = R.tiny_case()
    m = HF.hf_model(case["sd"])
    out = {"features_clip0": HF.hf_features(case["clips"][0])[::FEATURE_STRIDE].astype(np.float32)}
    P = len(R.TINY_SOT)
    for c, f in enumerate(case["feats"]):
        xa = HF.hf_encoder(m, f)                                  # the float64 features of the restatement: HF's own are float32
        out[f"encoder_rows_{c}"] = xa[list(ENC_ROWS)]
        toks = list(R.TINY_SOT) + case["free"][c][0]
        out[f"logits_{c}"] = HF.hf_logits(m, xa, toks[:-1])[P - 1:]
        out[f"greedy_{c}"] = np.array(HF.hf_greedy(m, xa, R.TINY_STEPS), np.int32)
        print(c, out[f"greedy_{c}"].tolist(), "restatement", case["free"][c][0])
    path = os.path.join(ROOT, "tests", "golden", "whisper_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
