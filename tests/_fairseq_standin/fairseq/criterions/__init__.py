import inspect

import torch.nn as nn

from fairseq.dataclass import FairseqDataclass

CRITERION_REGISTRY = {}
CRITERION_DATACLASS_REGISTRY = {}
CRITERION_CLASS_NAMES = set()


class FairseqCriterion(nn.Module):
    def __init__(self, task):
        super().__init__()
        self.task = task
        tgt = getattr(task, "target_dictionary", None)
        self.padding_idx = tgt.pad() if tgt is not None else -100

    @classmethod
    def build_criterion(cls, cfg, task):
        """Construct a criterion from its config: every constructor argument is `task`, `cfg`, a field of cfg, or defaulted."""
        init_args = {}
        for p in inspect.signature(cls).parameters.values():
            if p.kind in (p.POSITIONAL_ONLY, p.VAR_POSITIONAL, p.VAR_KEYWORD):
                raise NotImplementedError(f"{p.kind} is not supported")
            if p.name == "task":
                init_args["task"] = task
            elif p.name == "cfg":
                init_args["cfg"] = cfg
            elif hasattr(cfg, p.name):
                init_args[p.name] = getattr(cfg, p.name)
            elif p.default != p.empty:
                pass
            else:
                raise NotImplementedError(f"Unable to infer Criterion arguments, please implement {cls.__name__}.build_criterion")
        return cls(**init_args)

    def forward(self, model, sample, reduce=True):
        raise NotImplementedError

    @staticmethod
    def reduce_metrics(logging_outputs) -> None:
        raise NotImplementedError

    @staticmethod
    def logging_outputs_can_be_summed() -> bool:
        return False


def register_criterion(name, dataclass=None):
    def register_x_cls(cls):
        if name in CRITERION_REGISTRY:
            raise ValueError(f"Cannot register duplicate criterion ({name})")
        if cls.__name__ in CRITERION_CLASS_NAMES:
            raise ValueError(f"Cannot register criterion with duplicate class name ({cls.__name__})")
        if not issubclass(cls, FairseqCriterion):
            raise ValueError(f"{cls.__name__} must extend FairseqCriterion")
        if dataclass is not None and not issubclass(dataclass, FairseqDataclass):
            raise ValueError(f"Dataclass {dataclass} must extend FairseqDataclass")
        cls.__dataclass = dataclass
        CRITERION_REGISTRY[name] = cls
        CRITERION_CLASS_NAMES.add(cls.__name__)
        if dataclass is not None:
            CRITERION_DATACLASS_REGISTRY[name] = dataclass
            node = dataclass()
            node._name = name
        return cls
    return register_x_cls


def build_criterion(cfg, task):
    from fairseq.tasks import merge_with_parent
    name = cfg["_name"]
    dc = CRITERION_DATACLASS_REGISTRY[name]
    return CRITERION_REGISTRY[name].build_criterion(merge_with_parent(dc(), cfg), task)
