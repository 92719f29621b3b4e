"""Tiny instances of every root model, with synthetic weights, for the packed-state tests (CPU and GPU)."""
from lip2speech_unit_amd import ops, speech_units, weights
from lip2speech_unit_amd.conformer import ConformerConfig
from lip2speech_unit_amd.hubert import AVHubertConfig
from lip2speech_unit_amd.model import MultiTargetEncoderModel
from lip2speech_unit_amd.model_auto_avsr import AutoAVSRConfig, MultiTargetAutoAVSREncoderModel
from lip2speech_unit_amd.model_avhubert import MultiTargetAVHubertEncoderModel
from lip2speech_unit_amd.model_raven import MultiTargetRAVENEncoderModel, RAVENConfig
from lip2speech_unit_amd.vocoder import AttrDict, MelCodeGenerator

VOC_H = dict(resblock="1", upsample_rates=[5, 4, 2, 2, 2], upsample_kernel_sizes=[11, 8, 4, 4, 4],
             upsample_initial_channel=512, resblock_kernel_sizes=[3, 7, 11],
             resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_embeddings=200, embedding_dim=128,
             model_in_dim=336, embedder_dim=256, multispkr="_", num_mels=80, text_supervision=False)
VOC_H_TEXT = dict(VOC_H, text_supervision=True, num_embeddings_text=40, embedding_dim_text=13, model_in_dim=80 + 2 * 128 + 13)


def _head(ffn):
    return ConformerConfig(conformer_layers=1, **({} if ffn is None else {"conformer_ffn_embed_dim": ffn}))


def avhubert(ffn=64, dtype=ops.F16):
    """ffn=None keeps the conformer's feed-forward at its checkpoint width (what the GPU tests run)."""
    return MultiTargetAVHubertEncoderModel.build_model(dtype=dtype, w2v_cfg=AVHubertConfig(encoder_layers=1), conformer_cfg=_head(ffn))


ROOTS = {
    "multi_target_avhubert": avhubert,
    "multi_target": lambda: MultiTargetEncoderModel.build_model(dtype=ops.F16, conformer_cfg=_head(64)),
    "multi_target_auto_avsr": lambda: MultiTargetAutoAVSREncoderModel.build_model(
        dtype=ops.F16, encoder_cfg=AutoAVSRConfig(encoder_num_blocks=1, encoder_linear_units=64), conformer_cfg=_head(64)),
    "multi_target_raven": lambda: MultiTargetRAVENEncoderModel.build_model(
        dtype=ops.F16, encoder_cfg=RAVENConfig(encoder_num_blocks=1, encoder_linear_units=64), conformer_cfg=_head(64)),
    "speech_units": lambda: speech_units.HubertModel(speech_units.HubertConfig(encoder_layers=1)),
    "vocoder": lambda: MelCodeGenerator(AttrDict(VOC_H), dtype=ops.F16),
    "vocoder_text": lambda: MelCodeGenerator(AttrDict(VOC_H_TEXT), dtype=ops.F16),
}


def synth(model, seed):
    return weights.synth_state_dict(weights.spec_of(model), seed=seed)


def loaded(make, seed):
    m = make()
    m.load_state_dict(synth(m, seed))
    return m.eval()
