"""The fp32 reference-precision mode of stage 1 (L2S_F32 / ops.F32 / dtype=f32), host side: the constants of the three layers
agree, the switches reach the model builders, and the cross-compiled library answers for fp32 descriptors without a GPU."""
import ctypes
import os
import re

import pytest
import torch

from lip2speech_unit_amd import _lib, inference, model as model_mod, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "lip2speech_hip.h")).read()


def test_f32_code_is_2_in_header_binding_and_ops():
    m = re.search(r"enum\s*\{\s*L2S_F16\s*=\s*0\s*,\s*L2S_BF16\s*=\s*1\s*,\s*L2S_F32\s*=\s*(\d+)\s*\}", _header())
    assert m and int(m.group(1)) == 2
    assert _lib.F32 == 2 and ops.F32 == 2
    assert (_lib.F16, _lib.BF16) == (0, 1)          # the 16-bit codes did not move


def test_abi_version_is_16_everywhere():
    assert int(re.search(r"#define\s+L2S_ABI_VERSION\s+(\d+)", _header()).group(1)) == 16
    assert _lib.ABI_VERSION == 16
    assert _lib.load().l2s_abi_version() == 16


def test_dtype_round_trip():
    assert ops.torch_dtype(ops.F32) is torch.float32
    assert ops.dtype_code(torch.float32) == ops.F32
    for code in (ops.F16, ops.BF16, ops.F32):
        assert ops.dtype_code(ops.torch_dtype(code)) == code
    with pytest.raises(_lib.L2SError):
        ops.dtype_code(torch.float64)


@pytest.mark.parametrize("value,want", [("f32", 2), ("FP32", 2), ("float32", 2), ("bf16", 1), ("f16", 0), (None, 0)])
def test_env_dtype(monkeypatch, value, want):
    if value is None:
        monkeypatch.delenv("L2S_DTYPE", raising=False)
    else:
        monkeypatch.setenv("L2S_DTYPE", value)
    assert model_mod.env_dtype() == want


def test_parse_dtype_selects_fp32_for_stage_1_only():
    assert model_mod.parse_dtype("f32") == (ops.F32, ops.F16)      # the vocoder keeps fp16 operands
    assert model_mod.parse_dtype("bf16") == (ops.BF16, ops.BF16)
    assert model_mod.parse_dtype("f16") == (ops.F16, ops.F16)
    with pytest.raises(ValueError):
        model_mod.parse_dtype("f64")


class _Reached(Exception):
    pass


def test_cli_override_reaches_build_model(monkeypatch):
    cfg = inference.parse_overrides(["dtype=f32", "synthetic_weights=true"])
    assert cfg["dtype"] == "f32" and cfg["fp16"] is False         # fp16=false keeps its meaning: it is not the precision switch
    seen = {}

    def build_model(cls, task=None, dtype=None, **kw):
        seen["stage1"] = dtype
        raise _Reached

    monkeypatch.setattr(inference.MultiTargetAVHubertEncoderModel, "build_model", classmethod(build_model))
    with pytest.raises(_Reached):
        inference.build_model(cfg, task=None)
    assert seen["stage1"] == ops.F32

    from lip2speech_unit_amd import vocoder

    def voc_init(self, h, dtype=None, **kw):
        seen["vocoder"] = dtype
        raise _Reached

    monkeypatch.setattr(vocoder.MelCodeGenerator, "__init__", voc_init)
    import json
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".json") as f:
        json.dump({"num_mels": 80}, f)
        f.flush()
        cfg["vocoder.config"] = f.name
        with pytest.raises(_Reached):
            inference.build_vocoder(cfg)
    assert seen["vocoder"] == ops.F16


def test_build_model_accepts_f32_and_env(monkeypatch):
    from lip2speech_unit_amd.conformer import ConformerConfig
    from lip2speech_unit_amd.hubert import AVHubertConfig
    from lip2speech_unit_amd.model_avhubert import MultiTargetAVHubertEncoderModel
    small = dict(w2v_cfg=AVHubertConfig(encoder_layers=1), conformer_cfg=ConformerConfig(conformer_layers=1))
    m = MultiTargetAVHubertEncoderModel.build_model(dtype=ops.F32, **small)
    assert m.conformer.dtype == ops.F32 and m.encoder.w2v_model.dtype == ops.F32
    assert m.encoder.w2v_model.feature_extractor_video.resnet.dtype == ops.F32
    monkeypatch.setenv("L2S_DTYPE", "f32")
    m = MultiTargetAVHubertEncoderModel.build_model(**small)
    assert m.conformer.dtype == ops.F32


def test_other_model_families_name_fp32_when_they_refuse():
    from lip2speech_unit_amd.model import MultiTargetEncoderModel
    from lip2speech_unit_amd.model_auto_avsr import MultiTargetAutoAVSREncoderModel
    from lip2speech_unit_amd.model_raven import MultiTargetRAVENEncoderModel
    for cls in (MultiTargetEncoderModel, MultiTargetAutoAVSREncoderModel, MultiTargetRAVENEncoderModel):
        with pytest.raises(NotImplementedError, match="fp32"):
            cls.build_model(dtype=ops.F32)


def test_library_answers_for_fp32_descriptors():
    lib = _lib.load()
    d = _lib.GemmDesc(M=6400, N=4096, Cin=1024, ntaps=1, groups=1, dtype=_lib.F32)
    assert lib.l2s_tapgemm(ctypes.byref(d), None) == -1                       # L2S_EINVAL: null operands, nothing launched
    assert lib.l2s_tapgemm_variant(ctypes.byref(d)) == 2128128                # the fp32 kernel's own code (128 x 128 tile)
    assert lib.l2s_tapgemm_epilogue_family(ctypes.byref(d)) == 32
    d16 = _lib.GemmDesc(M=6400, N=4096, Cin=1024, ntaps=1, groups=1, dtype=_lib.F16)
    assert lib.l2s_tapgemm_variant(ctypes.byref(d16)) != 2128128
    assert 0 <= lib.l2s_tapgemm_epilogue_family(ctypes.byref(d16)) <= 9
    hdr = _header()
    assert int(re.search(r"#define\s+L2S_VARIANT_F32\s+(\d+)", hdr).group(1)) == 2128128
    assert int(re.search(r"#define\s+L2S_EPI_FAMILY_F32\s+(\d+)", hdr).group(1)) == 32
    # null pointers are refused for fp32 by the other entry points too
    assert lib.l2s_layernorm(None, 1, 0, None, None, 1e-5, None, 1, 0, None, 0, 1, 4, 0, None, 1, 0, _lib.F32, None) == -1
    assert lib.l2s_attention(None, 0, None, 0, None, 0, None, None, None, 1, 1, 1, 1, _lib.F32, None) == -1
