"""Host side of the `multi_target` criterion: registration (stand-alone and through the fairseq stand-in), the ABI / torch-op
surface of the three new entries, `aggregate`, the dataset's text labels and the validation CLI's parsing and batching.  No GPU."""
import math
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from lip2speech_unit_amd import _lib, ops, plugin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDIN = os.path.join(ROOT, "tests", "_fairseq_standin")
LABELS = os.path.join(ROOT, "tests", "golden", "lrs3_sample")
ENTRIES = ("l2s_unit_ce", "l2s_mel_l1_sc", "l2s_ctc_loss")


class _Dict:
    def pad(self):
        return 1


class _Task:
    target_dictionary = _Dict()

    def __init__(self, text=False):
        self.cfg = {"text_supervision": text}


def test_standalone_registration_and_build():
    from lip2speech_unit_amd import criterion
    from lip2speech_unit_amd.task import Lip2SpeechTask, decode_config
    cls, dc = plugin.CRITERION_REGISTRY["multi_target"]
    assert cls is criterion.MultiTargetCriterion and dc is criterion.MultiTargetCriterionConfig
    assert issubclass(cls, plugin.CriterionBase) and issubclass(dc, plugin.DataclassBase)
    d = dc()
    assert (d.label_smoothing, d.report_accuracy, d.ignore_prefix_size, d.sentence_avg, d.mel_weight) == (0.0, False, 0, False, 1.0)
    # the reference's constructor signature (criterion.py:26-34)
    import inspect
    assert list(inspect.signature(cls.__init__).parameters) == ["self", "task", "sentence_avg", "label_smoothing", "mel_weight",
                                                                "ignore_prefix_size", "report_accuracy"]
    task = Lip2SpeechTask(decode_config(data=LABELS, label_dir=LABELS))
    c = task.build_criterion({"_name": "multi_target", "label_smoothing": 0.1, "mel_weight": 10, "report_accuracy": True})
    assert type(c) is cls and (c.eps, c.mel_weight, c.report_accuracy, c.sentence_avg, c.padding_idx) == (0.1, 10.0, True, False, 1)
    assert c.text_supervision is False
    with pytest.raises(KeyError):
        task.build_criterion({"_name": "multi_target", "not_a_field": 1})
    with pytest.raises(KeyError):
        task.build_criterion({"_name": "no_such_criterion"})
    with pytest.raises(NotImplementedError, match="ignore_prefix_size"):
        task.build_criterion({"_name": "multi_target", "ignore_prefix_size": 1})
    with pytest.raises(NotImplementedError, match="text print"):
        c.log_text_sample()
    with pytest.raises(NotImplementedError, match="reduce=False"):
        c.forward(None, {}, reduce=False)


def test_fairseq_mode_registers_and_builds_through_the_standin():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([STANDIN, ROOT, os.environ.get("PYTHONPATH", "")]))
    code = f"""
        import fairseq.criterions as fc
        from fairseq.dataclass import FairseqDataclass
        from lip2speech_unit_amd import plugin, criterion, task
        assert plugin.HAVE_FAIRSEQ and plugin.CriterionBase is fc.FairseqCriterion
        assert fc.CRITERION_REGISTRY["multi_target"] is criterion.MultiTargetCriterion
        assert fc.CRITERION_DATACLASS_REGISTRY["multi_target"] is criterion.MultiTargetCriterionConfig
        assert issubclass(criterion.MultiTargetCriterion, fc.FairseqCriterion)
        assert issubclass(criterion.MultiTargetCriterionConfig, FairseqDataclass)
        assert criterion.MultiTargetCriterionConfig().sentence_avg == "${{optimization.sentence_avg}}"
        t = task.Lip2SpeechTask(task.decode_config(data={LABELS!r}, label_dir={LABELS!r}))
        c = fc.build_criterion({{"_name": "multi_target", "label_smoothing": 0.1, "mel_weight": 10, "report_accuracy": True}}, t)
        assert type(c) is criterion.MultiTargetCriterion and c.task is t
        assert (c.eps, c.mel_weight, c.report_accuracy, c.padding_idx) == (0.1, 10.0, True, 1)
        try:
            @plugin.register_criterion("not_a_criterion")
            class NotACriterion:
                pass
        except ValueError as e:
            assert "must extend FairseqCriterion" in str(e)
        else:
            raise AssertionError("registration of a non-FairseqCriterion must raise")
        try:
            @plugin.register_criterion("bad_dataclass", dataclass=dict)
            class C2(fc.FairseqCriterion):
                pass
        except ValueError as e:
            assert "must extend FairseqDataclass" in str(e)
        else:
            raise AssertionError("a dataclass outside FairseqDataclass must raise")
        assert set(plugin.CRITERION_REGISTRY) == {{"multi_target"}}
        print("CRITERION-FAIRSEQ-OK")
    """
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CRITERION-FAIRSEQ-OK" in r.stdout, r.stdout + r.stderr


def test_abi_surface_of_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "lip2speech_hip.h")).read()
    assert re.search(r"#define\s+L2S_ABI_VERSION\s+16\b", hdr) and _lib.ABI_VERSION == 16
    for e in ENTRIES + ("l2s_ctc_loss_workspace",):
        assert re.search(r"\b%s\s*\(" % e, hdr) and e in _lib.SIGNATURES, e
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % e, hdr).group(1)
        assert len(_lib.SIGNATURES[e][0]) == len(decl.split(",")), e            # one ctypes type per declared argument
    assert "l2s_ctc_loss_workspace" in ops.HOST_QUERIES
    for e in ENTRIES:
        name = e[4:]
        assert ops.ENTRY_OF[name] == e
        schema = str(getattr(torch.ops.lip2speech, name).default._schema)
        assert schema.rstrip().endswith("-> ()") and "!" in schema
    with pytest.raises(ops.L2SError):                    # no CPU path
        ops.unit_ce(torch.zeros(4, 8), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1), torch.zeros(1),
                    torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), B=1, T2=4, V=8)


def test_fake_tensor_shapes_of_the_new_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        dev = "cuda"
        f = lambda *s: torch.empty(*s, device=dev)                                  # noqa: E731
        i = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)               # noqa: E731
        nll, sm, ok, n = f(3), f(3), i(3), i(3)
        assert torch.ops.lip2speech.unit_ce(f(3 * 10, 204), i(3, 9), nll, sm, ok, n, B=3, T2=10, V=204, lens=i(3)) is None
        assert nll.shape == (3,) and ok.dtype == torch.int32
        assert torch.ops.lip2speech.mel_l1_sc(f(3, 20, 80), f(3, 22, 80), f(3), f(3), f(3), i(3), B=3, Tm_pred=20, Tm_targ=22,
                                              crop_len=20, lens=i(3)) is None
        assert torch.ops.lip2speech.ctc_loss(f(3 * 10, 4000), i(7), i(3), i(3), f(3 * 10 * 5), f(3), B=3, L=10, V=4000,
                                             S_max=4, lens=i(3)) is None


def test_aggregate_base2_ppl_accuracy():
    from lip2speech_unit_amd.criterion import MultiTargetCriterion as C
    logs = [{"loss": 40.0, "nll_loss": 12.0, "mel_loss": 6.0, "ctc_loss": 3.0, "ntokens": 10, "nsentences": 2, "sample_size": 2,
             "n_correct": 3, "total": 9},
            {"loss": torch.tensor(20.0), "nll_loss": torch.tensor(8.0), "mel_loss": 2.0, "ctc_loss": 1.0, "ntokens": 6,
             "nsentences": 2, "sample_size": 2, "n_correct": torch.tensor(4), "total": torch.tensor(5)}]
    a = C.aggregate(logs)
    assert a["loss"] == pytest.approx(60.0 / 4 / math.log(2), rel=1e-15)          # per sample_size, base 2
    assert a["nll_loss"] == pytest.approx(20.0 / 16 / math.log(2), rel=1e-15)      # per token, base 2
    assert a["ppl"] == pytest.approx(2 ** a["nll_loss"], rel=1e-15) and a["ppl"] == pytest.approx(math.exp(20.0 / 16), rel=1e-12)
    assert a["accuracy"] == pytest.approx(100.0 * 7 / 14, rel=1e-15)
    assert a["mel_loss"] == pytest.approx(8.0 / 4) and a["ctc_loss"] == pytest.approx(4.0 / 4)
    b = C.aggregate([{"loss": 1.0, "nll_loss": 1.0, "mel_loss": None, "ntokens": 1, "sample_size": 1}])
    assert set(b) == {"loss", "nll_loss", "ppl"}
    from tests import _criterion_reference as R
    assert R.reduce_metrics([{k: float(v) for k, v in log.items()} for log in logs]) == pytest.approx(a, rel=1e-15)
    assert C.logging_outputs_can_be_summed()
    C.reduce_metrics(logs)            # without fairseq's meters: nothing to log into, and no error


def test_dataset_text_labels(tmp_path):
    from lip2speech_unit_amd.data import MultiTargetDataset
    from lip2speech_unit_amd.task import Lip2SpeechTask, decode_config
    from tests._synth_dataset import make
    lab = make(str(tmp_path / "ds"), frames=(6, 4, 3))
    plain = MultiTargetDataset(os.path.join(lab, "test.tsv"), label_path=os.path.join(lab, "test.unt"))
    assert plain.text_labels is None and "text_labels" not in plain.collater([plain[0], plain[1]])
    missing = MultiTargetDataset(os.path.join(lab, "test.tsv"), text_label_path=os.path.join(lab, "nope.txt"))
    assert missing.text_labels is None                       # absent file: unchanged behaviour
    with open(os.path.join(lab, "test.txt"), "w") as f:
        f.write("5 5 9\n\n7 8 9 10\n")                       # the second clip has an empty target
    ds = MultiTargetDataset(os.path.join(lab, "test.tsv"), label_path=os.path.join(lab, "test.unt"),
                            text_label_path=os.path.join(lab, "test.txt"))
    b = ds.collater([ds[2], ds[1], ds[0]])
    assert b["text_labels"].dtype == torch.int32 and b["text_labels"].tolist() == [7, 8, 9, 10, 5, 5, 9]
    assert b["text_labels_lengths"].dtype == torch.int32 and b["text_labels_lengths"].tolist() == [4, 0, 3]
    assert not b["text_labels_lengths"].is_cuda
    with open(os.path.join(lab, "short.txt"), "w") as f:
        f.write("1\n")
    with pytest.raises(AssertionError):
        MultiTargetDataset(os.path.join(lab, "test.tsv"), text_label_path=os.path.join(lab, "short.txt"))
    # the task wires <label_dir>/<split>.txt in only under text supervision
    t = Lip2SpeechTask(decode_config(data=lab, label_dir=lab))
    assert t.load_dataset("test").text_labels is None
    t.cfg.text_supervision = True
    assert len(t.load_dataset("test").text_labels) == 3


def test_validate_cli_parsing_and_batches():
    from lip2speech_unit_amd import validate as v
    cfg = v.parse_overrides(["common_eval.path=x.pt", "dataset.gen_subset=val"])
    assert cfg["dataset.max_tokens"] == 3600 and cfg["dataset.batch_size"] is None and cfg["dataset.gen_subset"] == "val"
    assert v.criterion_config(cfg) == {"_name": "multi_target", "label_smoothing": 0.1, "mel_weight": 10.0, "report_accuracy": True,
                                       "ignore_prefix_size": 0, "sentence_avg": True}
    cfg = v.parse_overrides(["optimization.sentence_avg=false", "criterion.mel_weight=1", "dtype=f32", "dataset.batch_size=1",
                             "synthetic_weights=true"])
    assert cfg["criterion.sentence_avg"] is False and cfg["criterion.mel_weight"] == 1 and cfg["dtype"] == "f32"
    assert cfg["dataset.batch_size"] == 1 and cfg["synthetic_weights"] is True
    assert v.parse_overrides(["criterion.sentence_avg=false"])["criterion.sentence_avg"] is False
    for bad in (["--beam", "5"], ["positional"], ["criterion.no_such=1"]):
        with pytest.raises(SystemExit):
            v.parse_overrides(bad)
    sizes = [50, 100, 30, 100, 70, 10]
    assert v.form_batches(sizes, None, 1) == [[1], [3], [4], [0], [2], [5]]             # longest first, ties in manifest order
    assert v.form_batches(sizes, 200, None) == [[1, 3], [4, 0], [2, 5]]                  # clips x longest <= 200
    assert v.form_batches(sizes, 3600, None) == [[1, 3, 4, 0, 2, 5]]
    assert v.form_batches(sizes, 3600, 4) == [[1, 3, 4, 0], [2, 5]]
    assert v.form_batches(sizes, 100, 4) == [[1], [3], [4], [0, 2], [5]]
    for mt, bs in ((200, None), (100, 4), (3600, 2)):
        bt = v.form_batches(sizes, mt, bs)
        assert sorted(i for b in bt for i in b) == list(range(6))
        assert all(len(b) * max(sizes[i] for i in b) <= mt and (bs is None or len(b) <= bs) for b in bt)
    with pytest.raises(ValueError):
        v.form_batches(sizes, 99, None)
    assert v.format_line({"loss": 1.23456, "nll_loss": 2.0, "ppl": 4.0, "accuracy": 50.0, "mel_loss": 0.5}) == \
        "valid | loss 1.235 | nll_loss 2.000 | ppl 4.00 | accuracy 50.000 | mel_loss 0.50000"
    assert v.format_line({"loss": 1.0, "nll_loss": 2.0, "ppl": 4.0, "mel_loss": 0.5, "ctc_loss": 0.25}).endswith("| ctc_loss 0.25000")
