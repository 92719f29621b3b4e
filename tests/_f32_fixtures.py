"""The reference-pinned fixtures of the fp32 checks (tests/test_f32_models_gpu.py): what each holds, the state dict and inputs
it was made with, and an fp64 evaluation of the same module on the CPU (the oracles run unchanged on a `.double()` state dict:
oracle/frontend.py, oracle/conformer.py, oracle/avhubert.py hard-code no dtype).

The fixture is the reference's own float32 output; its distance from the fp64 evaluation is the reference's fp32 rounding as
frozen in the file.  The tolerance of a check is 4 x that distance, floor 2^-20 * max|golden| - nothing from the GPU enters."""
import os

import numpy as np
import torch

from lip2speech_unit_amd import weights


def _d64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def tolerance(gold, ref64):
    dev = (gold.double() - ref64).abs().max().item()
    scale = gold.abs().max().item()
    return max(4.0 * dev, 2.0 ** -20 * scale), dev, scale


def frontend(golden_dir):
    """-> dict(sd, x [1,1,6,88,88] fp32, gold / ref64 of `out` [1,512,6] and `stem_t2` [64,44,44])."""
    from lip2speech_unit_amd.resnet import ResEncoder
    from oracle import frontend as ofe
    d = np.load(os.path.join(golden_dir, "frontend.npz"))
    sd = weights.synth_state_dict(weights.spec_of(ResEncoder("prelu", None)), seed=int(d["seed"]))
    x = ((torch.from_numpy(d["frames_u8"]).float() / 255.0 - 0.421) / 0.165).unsqueeze(1)
    taps = {}
    with torch.no_grad():
        # the frames are normalised in float32 first, as the reference's dataset code does; the module runs in fp64 from there
        out64 = ofe.res_encoder(_d64(sd), x.double(), taps)
    return {"sd": sd, "x": x,
            "out": (torch.from_numpy(d["out"]), out64),
            "stem_t2": (torch.from_numpy(d["stem_t2"].astype(np.float32)), taps["stem"][0, :, 2])}


def conformer(golden_dir):
    """-> dict(esd (Conformer().encoder state dict), x [2,70,512], lens, gold / ref64 of `out[0]` [70,512] (clip 0 fills the
    batch) and `out_clip1_alone` [44,512])."""
    from lip2speech_unit_amd.conformer import Conformer
    from oracle import conformer as oc
    d = np.load(os.path.join(golden_dir, "conformer.npz"))
    esd = weights.synth_state_dict(weights.spec_of(Conformer().encoder), seed=int(d["seed"]))
    sd64 = _d64({"e." + k: v for k, v in esd.items()})
    x = torch.from_numpy(d["x"])
    lens = torch.from_numpy(d["lens"])
    n = int(lens[1])
    T = x.shape[1]
    with torch.no_grad():
        y0, _ = oc.espnet_encoder_after_frontend(sd64, "e", x[0:1].double(), torch.ones(1, 1, T, dtype=torch.bool))
        y1, _ = oc.espnet_encoder_after_frontend(sd64, "e", x[1:2, :n].double(), torch.ones(1, 1, n, dtype=torch.bool))
    return {"esd": esd, "x": x, "lens": lens,
            "out0": (torch.from_numpy(d["out"])[0], y0[0]),
            "out_clip1_alone": (torch.from_numpy(d["out_clip1_alone"])[0], y1[0])}


def hubert_standin(golden_dir):
    """-> dict(sd ("enc."-prefixed TransformerEncoder state dict), layers, x [2,30,1024], lens, pad, gold / ref64 of `out`)."""
    from lip2speech_unit_amd.hubert import AVHubertConfig, TransformerEncoder
    from oracle import avhubert as oa
    d = np.load(os.path.join(golden_dir, "hubert_standin.npz"))
    L = int(d["layers"])
    spec = weights.spec_of(TransformerEncoder(AVHubertConfig(encoder_layers=L)))
    sd = weights.synth_state_dict([("enc." + k, s) for k, s in spec], seed=int(d["seed"]))
    x = torch.from_numpy(d["x"])
    lens = torch.from_numpy(d["lens"])
    pad = torch.arange(x.shape[1])[None, :] >= lens[:, None]
    with torch.no_grad():
        y = oa.transformer_encoder(_d64(sd), "enc", x.double(), pad, layers=L)
    return {"sd": sd, "layers": L, "x": x, "lens": lens, "pad": pad, "out": (torch.from_numpy(d["out"]), y)}


def all_fixture_references(golden_dir):
    f, c, h = frontend(golden_dir), conformer(golden_dir), hubert_standin(golden_dir)
    valid = ~h["pad"]
    return {"frontend.out": f["out"], "frontend.stem_t2": f["stem_t2"], "conformer.out[0]": c["out0"],
            "conformer.out_clip1_alone": c["out_clip1_alone"],
            "hubert_standin.out": (h["out"][0][valid], h["out"][1][valid])}
