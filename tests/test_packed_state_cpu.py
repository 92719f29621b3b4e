"""The packed-state protocol (packing.PackedState) without a GPU: who holds packed weights, what a load_state_dict anywhere in
the tree invalidates, the two stale-weight cases it fixes, packed() / state_epoch / GraphCache(state=...) behaviour."""
import copy
import pickle

import pytest
import torch

from lip2speech_unit_amd import ops, speaker_encoder
from lip2speech_unit_amd.conformer import Encoder
from lip2speech_unit_amd.packing import PackedState, state_epoch
from lip2speech_unit_amd.pipeline import GraphCache
from tests import _tiny_models as tiny


@pytest.fixture(scope="module", params=list(tiny.ROOTS))
def root(request):
    return tiny.loaded(tiny.ROOTS[request.param], seed=0)


@pytest.fixture(scope="module")
def avhubert():
    return tiny.loaded(tiny.avhubert, seed=0)


def holders(m):
    return [d for d in m.modules() if hasattr(d, "_packed")]


def packed_cpu(d):
    return d.packed("cpu", dtype=ops.F16) if isinstance(d, Encoder) else d.packed("cpu")


def test_every_holder_follows_the_protocol(root):
    hs = holders(root)
    assert hs and all(isinstance(d, PackedState) for d in hs)


def test_a_load_invalidates_the_holders_below_it_and_no_other(root):
    """For every module `a` with a holder below it (or itself one): a.load_state_dict drops the packed and the derived state of
    exactly the holders under `a`; every other holder keeps the identical objects."""
    hs = holders(root)
    for a in root.modules():
        below = [d for d in a.modules() if hasattr(d, "_packed")]
        if not below:
            continue
        for d in hs:                                   # (a parent's pack may re-pack a child: note the objects afterwards)
            packed_cpu(d)
            d.derived("probe", object)
        before = {d: (d._packed, d._derived["probe"]) for d in hs}
        assert all(p is not None for p, _ in before.values())
        sd = a.state_dict()
        a.load_state_dict(sd)
        for d in hs:
            if d in below:
                assert d._packed is None and d._derived == {}, (type(a).__name__, type(d).__name__)
            else:
                assert d._packed is before[d][0] and d._derived["probe"] is before[d][1], (type(a).__name__, type(d).__name__)


def test_loading_into_the_transformer_child_alone_repacks_it(avhubert):
    te = avhubert.encoder.w2v_model.encoder
    old = packed_cpu(te)["layers"][0]["wo"].clone()
    sd = tiny.synth(te, seed=1)
    te.load_state_dict(sd)
    new = packed_cpu(te)["layers"][0]["wo"]
    assert torch.equal(new, sd["layers.0.self_attn.out_proj.weight"].to(torch.float16))
    assert not torch.equal(new, old)


@pytest.mark.parametrize("h", [tiny.VOC_H, tiny.VOC_H_TEXT], ids=["plain", "text"])
def test_vocoder_reload_rebuilds_the_precise_state(h):
    from lip2speech_unit_amd.vocoder import AttrDict, MelCodeGenerator
    g = tiny.loaded(lambda: MelCodeGenerator(AttrDict(h), dtype=ops.F16), seed=0)
    assert g._precise_state("cpu") is g._precise_state(torch.device("cpu"))
    old_front = g._precise_front("cpu")
    sd = tiny.synth(g, seed=1)
    g.load_state_dict(sd)
    P, F = g._precise_state("cpu"), g._precise_front("cpu")
    assert torch.equal(P["pre_b"], sd["conv_pre.bias"]) and torch.equal(F["fc_b"], sd["fc.bias"])
    hi, lo = F["sp"]
    assert torch.equal(hi, sd["spkr.weight"].to(torch.float16)) and F is not old_front
    assert torch.equal(lo, (sd["spkr.weight"] - hi.float()).to(torch.float16))
    g.remove_weight_norm()                              # edits the parameters in place: drops the state as a load does
    assert g._derived == {} and g._packed is None


def test_packed_returns_one_object_per_device(avhubert):
    for d in holders(avhubert):
        d.invalidate()
        P = packed_cpu(d)
        assert packed_cpu(d) is P
    con = avhubert.conformer
    con.pack("cpu")
    P = con._packed
    assert con.packed(torch.device("cpu")) is P and "dev_probe" not in P


def test_transformer_encoder_packs_as_many_layers_as_asked():
    from lip2speech_unit_amd.hubert import TransformerEncoder
    from lip2speech_unit_amd.speech_units import HubertConfig
    te = TransformerEncoder(HubertConfig(encoder_layers=6, encoder_embed_dim=64, encoder_ffn_embed_dim=64, encoder_attention_heads=1),
                            dtype=ops.F32)
    P = te.packed("cpu", n_layers=2)
    assert len(P["layers"]) == 2
    assert te.packed("cpu", n_layers=1) is P            # two layers cover one
    P6 = te.packed("cpu", n_layers=6)
    assert P6 is not P and len(P6["layers"]) == 6
    assert te.packed("cpu") is P6                       # no n_layers: all of them


def test_conformer_encoder_repacks_for_another_operand_type(avhubert):
    enc = avhubert.conformer.encoder
    P = enc.packed("cpu", dtype=ops.F16)
    assert enc.packed("cpu", dtype=ops.F16) is P
    Q = enc.packed("cpu", dtype=ops.BF16)
    assert Q is not P and Q["w_emb"].dtype == torch.bfloat16


def test_state_epoch_moves_forward_only(avhubert):
    seen = [state_epoch(avhubert)]

    def moved():
        seen.append(state_epoch(avhubert))
        assert seen[-1] > max(seen[:-1]), seen
    res = avhubert.encoder.w2v_model.feature_extractor_video.resnet
    res.invalidate()
    moved()
    res.pack("cpu")
    moved()
    res.pack("cpu")                                     # a repack replaces the object
    moved()
    avhubert.conformer.encoder.load_state_dict(avhubert.conformer.encoder.state_dict())
    moved()
    assert state_epoch(avhubert) == seen[-1]            # reading it does not move it
    assert state_epoch(avhubert.conformer) <= seen[-1] and state_epoch(torch.nn.Linear(2, 2)) == 0


def test_a_deep_copy_invalidates_itself(avhubert):
    for d in holders(avhubert):
        packed_cpu(d)
    twin = copy.deepcopy(avhubert)
    assert all(d._packed is not None for d in holders(twin))
    twin.load_state_dict(twin.state_dict())
    assert all(d._packed is None for d in holders(twin))
    assert all(d._packed is not None for d in holders(avhubert))
    assert state_epoch(twin) > state_epoch(avhubert)


def test_models_still_pickle(avhubert):
    for d in holders(avhubert):
        packed_cpu(d)
    twin = pickle.loads(pickle.dumps(avhubert))
    twin.load_state_dict(twin.state_dict())             # the hook came along
    assert all(d._packed is None for d in holders(twin))


def test_speaker_encoder_drops_its_operands_on_load_and_refuses_the_cpu():
    enc = speaker_encoder.SpeakerEncoder()
    assert isinstance(enc, PackedState)
    probe = enc.derived(0, object)
    assert enc.derived(0, object) is probe
    enc.load_state_dict(speaker_encoder.synthetic_state_dict())
    assert enc._derived == {}
    with pytest.raises(ops.L2SError):
        enc.pack("cpu")


def test_graph_cache_drops_its_entries_when_the_state_moves():
    """No capture here: the entries are stand-ins, and the call stops at the first thing that needs a device."""
    state = [1]
    cache = GraphCache(lambda x: x, state=lambda: state[0])
    cache._drop_if_state_changed()
    cache.entries["k"] = "capture"
    cache._drop_if_state_changed()
    assert cache.entries == {"k": "capture"}
    state[0] = 2

    class Stop(Exception):
        pass

    class T:                                             # a "tensor" whose first use past the state check raises
        @property
        def shape(self):
            raise Stop
    with pytest.raises(Stop):
        cache(T())
    assert cache.entries == {}
    plain = GraphCache(lambda x: x)
    plain.entries["k"] = "capture"
    plain._drop_if_state_changed()
    assert plain.entries == {"k": "capture"}
