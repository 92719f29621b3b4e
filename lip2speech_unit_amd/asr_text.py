"""The text side of the Whisper recogniser (whisper.py), all host code: the decoding configuration (which ids are forced,
forbidden and final), the detokeniser (ids -> text from a vocabulary file) and the word error rate the reference publishes
(its `README.md:103-122`; formula at `multi_target_lip2speech/inference_server.py:364-373` and `avhubert/infer_s2s.py:258`:
pooled word edit distance over the pooled reference word count)."""
import base64
import json
import re
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

# openai-whisper's LANGUAGES, in the order its tokenizer numbers the language tokens
LANGUAGES = ("en zh de es ru ko fr ja pt tr pl ca nl ar sv it id hi fi vi he uk el ms cs ro da hu ta no th ur hr bg lt la mi ml cy sk te "
             "fa lv bn sr az sl kn et mk br eu is hy ne mn bs kk sq sw gl mr pa si km sn yo so af oc ka be tg sd gu am yi lo uz fo ht ps "
             "tk nn mt sa lb my bo tl mg as tt haw ln ha ba jw su yue").split()


def special_ids(n_vocab: int) -> Dict[str, int]:
    """The special ids openai-whisper's tokenizer derives from the vocabulary size: 51 864 = the English-only models (GPT-2's
    50 256 ranks, then eot), 51 865 = multilingual with 99 language tokens, 51 866 = with 100 (large-v3).  Order after the text
    ranks: eot, sot, the languages, translate, transcribe, startoflm, startofprev, nospeech, notimestamps, 1 501 timestamps."""
    if n_vocab == 51864:
        eot, n_lang = 50256, 99
    elif n_vocab in (51865, 51866):
        eot, n_lang = 50257, n_vocab - 51766
    else:
        raise ValueError(f"n_vocab = {n_vocab}: not a Whisper vocabulary (51864, 51865 or 51866); pass the ids explicitly")
    sot = eot + 1
    ids = {"eot": eot, "sot": sot, "lang0": sot + 1, "n_lang": n_lang}
    for i, name in enumerate(("translate", "transcribe", "startoflm", "startofprev", "nospeech", "notimestamps")):
        ids[name] = sot + 1 + n_lang + i
    ids["timestamp0"] = ids["notimestamps"] + 1
    assert ids["timestamp0"] + 1501 == n_vocab
    return ids


@dataclass
class WhisperDecodeConfig:
    """Every id the greedy loop uses is an input: the forced prefix, the end token, the ids that may never be chosen and the ids
    that may not be chosen at the first sampled position."""
    sot_sequence: Tuple[int, ...]
    eot: int
    suppress: Tuple[int, ...] = ()
    begin_suppress: Tuple[int, ...] = ()
    max_new_tokens: int = 224
    special_start: Optional[int] = None          # ids from here on are not text (the detokeniser drops them)

    @classmethod
    def _from_specials(cls, s, prefix, non_speech, n_vocab, max_new_tokens):
        # openai-whisper's SuppressTokens (the "-1" list: non-speech symbols + these specials); the timestamps follow because
        # timestamp rules are out of scope: without them nothing else would keep a timestamp from being chosen
        sup = set(int(i) for i in non_speech)
        sup |= {s["sot"], s["translate"], s["transcribe"], s["startoflm"], s["startofprev"], s["nospeech"], s["notimestamps"]}
        sup |= set(range(s["lang0"], s["lang0"] + s["n_lang"])) | set(range(s["timestamp0"], n_vocab))
        return cls(sot_sequence=tuple(prefix), eot=s["eot"], suppress=tuple(sorted(sup)), begin_suppress=(220, s["eot"]),
                   max_new_tokens=max_new_tokens, special_start=s["eot"])

    @classmethod
    def english(cls, non_speech: Sequence[int] = (), max_new_tokens: int = 224):
        """The English-only models (base.en, ...): prefix sot, notimestamps; 220 is the blank the first position may not be.
        non_speech: openai-whisper's non_speech_tokens (derived from the BPE itself, e.g. a generation_config.json's
        suppress_tokens); left empty, punctuation-only ids stay allowed."""
        s = special_ids(51864)
        return cls._from_specials(s, (s["sot"], s["notimestamps"]), non_speech, 51864, max_new_tokens)

    @classmethod
    def multilingual(cls, language: str = "en", n_vocab: int = 51865, non_speech: Sequence[int] = (), max_new_tokens: int = 224):
        s = special_ids(n_vocab)
        if language not in LANGUAGES[: s["n_lang"]]:
            raise ValueError(f"language {language!r} is not one of the model's {s['n_lang']} language tokens")
        return cls._from_specials(s, (s["sot"], s["lang0"] + LANGUAGES.index(language), s["transcribe"], s["notimestamps"]), non_speech,
                                  n_vocab, max_new_tokens)

    @classmethod
    def from_generation_config(cls, path_or_dict, max_new_tokens: int = 224):
        """A HuggingFace generation_config.json: decoder_start_token_id + forced_decoder_ids (position, id) make the prefix."""
        g = path_or_dict if isinstance(path_or_dict, dict) else json.load(open(path_or_dict))
        prefix = [int(g["decoder_start_token_id"])]
        for pos, tok in sorted((int(p), t) for p, t in (g.get("forced_decoder_ids") or [])):
            if tok is None or pos != len(prefix):
                raise ValueError("forced_decoder_ids must name consecutive positions from 1 (set the language and task explicitly)")
            prefix.append(int(tok))
        eot = g["eos_token_id"]
        eot = int(eot[0] if isinstance(eot, (list, tuple)) else eot)
        return cls(sot_sequence=tuple(prefix), eot=eot, suppress=tuple(int(i) for i in g.get("suppress_tokens") or ()),
                   begin_suppress=tuple(int(i) for i in g.get("begin_suppress_tokens") or ()), max_new_tokens=max_new_tokens,
                   special_start=eot)


# ---- detokeniser -------------------------------------------------------------------------------------------------------------------

def _gpt2_byte_decoder() -> Dict[str, int]:
    """GPT-2's printable stand-ins for the 256 byte values (the alphabet of a byte-level vocab.json), inverted."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    chars, n = keep[:], 0
    codes = keep[:]
    for b in range(256):
        if b not in keep:
            codes.append(b)
            chars.append(256 + n)
            n += 1
    return {chr(c): b for c, b in zip(chars, codes)}


_SPECIAL = re.compile(r"^<\|.*\|>$")


@dataclass
class Detokenizer:
    """ids -> text.  `table[id]` is the token's bytes; ids that are not in the table, or at / past special_start, are dropped; the
    bytes of all kept tokens are joined BEFORE UTF-8 decoding, so a character split over tokens survives."""
    table: Dict[int, bytes] = field(default_factory=dict)
    special_start: Optional[int] = None

    @classmethod
    def from_tiktoken(cls, path, special_start=None):
        """openai-whisper's `.tiktoken` file: one `base64(token) rank` per line."""
        table = {}
        for line in open(path, "rb").read().splitlines():
            if line.strip():
                tok, rank = line.split()
                table[int(rank)] = base64.b64decode(tok)
        return cls(table, special_start)

    @classmethod
    def from_vocab_json(cls, path, special_start=None):
        """HuggingFace's byte-level `vocab.json` ({token string: id}); `<|...|>` entries are special."""
        dec = _gpt2_byte_decoder()
        table = {}
        for tok, i in json.load(open(path, encoding="utf-8")).items():
            if _SPECIAL.match(tok) or any(c not in dec for c in tok):
                continue
            table[int(i)] = bytes(dec[c] for c in tok)
        return cls(table, special_start)

    @classmethod
    def load(cls, path, special_start=None):
        return (cls.from_vocab_json if str(path).endswith(".json") else cls.from_tiktoken)(path, special_start)

    def decode(self, ids) -> str:
        lim = self.special_start
        return b"".join(self.table[int(i)] for i in ids if int(i) in self.table and (lim is None or int(i) < lim)).decode("utf-8", "replace")


# ---- word error rate ---------------------------------------------------------------------------------------------------------------

_NOT_WORD = re.compile(r"[^\w\s']|_")


def normalize_text(s: str) -> str:
    """Lower case; apostrophes kept; every other punctuation mark becomes a space; white space collapsed.  (Whisper's
    EnglishTextNormalizer - number and spelling rules - is not built.)"""
    return " ".join(_NOT_WORD.sub(" ", s.lower().replace("’", "'")).split())


def edit_distance(a: List[str], b: List[str]) -> int:
    """Word-level Levenshtein distance."""
    prev = list(range(len(b) + 1))
    for i, wa in enumerate(a, 1):
        cur = [i]
        for j, wb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (wa != wb)))
        prev = cur
    return prev[-1]


def wer(refs: Sequence[str], hyps: Sequence[str]) -> dict:
    """100 * sum(errors) / sum(reference words), pooled over the clips as the reference pools it.  Returns {"wer", "n_err",
    "n_total", "clips": [{"ref", "hyp", "errors", "words"}]} on the normalised texts; wer is None when there is no reference word."""
    if len(refs) != len(hyps):
        raise ValueError(f"{len(refs)} references for {len(hyps)} hypotheses")
    clips, n_err, n_total = [], 0, 0
    for r, h in zip(refs, hyps):
        r, h = normalize_text(r), normalize_text(h)
        e = edit_distance(h.split(), r.split())
        clips.append({"ref": r, "hyp": h, "errors": e, "words": len(r.split())})
        n_err += e
        n_total += len(r.split())
    return {"wer": 100.0 * n_err / n_total if n_total else None, "n_err": n_err, "n_total": n_total, "clips": clips}


class FairseqDictionary:
    """fairseq's Dictionary as the lip reader's target side uses it (`dict.wrd.txt`: one `<symbol> <count>` line per sentencepiece
    unit).  Ids 0 .. 3 are `<s> <pad> </s> <unk>` (nspecial = 4), the file's symbols follow in order.  `string` undoes the
    sentencepiece segmentation the way fairseq's `post_process="sentencepiece"` does; no sentencepiece model is needed."""
    BOS, PAD, EOS, UNK = 0, 1, 2, 3
    SPECIALS = ("<s>", "<pad>", "</s>", "<unk>")

    def __init__(self, symbols: Sequence[str] = ()):
        self.symbols = list(self.SPECIALS)
        self.nspecial = len(self.symbols)
        self.symbols.extend(symbols)
        self.index = {}
        for i, s in enumerate(self.symbols):
            self.index.setdefault(s, i)

    @classmethod
    def load(cls, path):
        syms = []
        with open(path, encoding="utf-8") as f:
            for ln in f:
                ln = ln.rstrip("\n")
                if not ln:
                    continue
                if ln.endswith(" #fairseq:overwrite"):
                    ln = ln[:-len(" #fairseq:overwrite")]
                sym, _, cnt = ln.rpartition(" ")
                if not sym or not cnt.lstrip("-").isdigit():
                    raise ValueError(f"{path}: expected '<symbol> <count>', got {ln!r}")
                syms.append(sym)
        return cls(syms)

    def __len__(self):
        return len(self.symbols)

    def pad(self):
        return self.PAD

    def eos(self):
        return self.EOS

    def unk(self):
        return self.UNK

    def encode_pieces(self, pieces: Sequence[str]) -> List[int]:
        return [self.index.get(p, self.UNK) for p in pieces]

    def string(self, ids: Sequence[int]) -> str:
        """Text of a hypothesis: eos, pad and the initial bos dropped, `<unk>` kept as fairseq prints it, then
        "".join(pieces).replace(" ", "").replace("▁", " ").strip()."""
        pieces = [self.symbols[int(i)] for i in ids if int(i) not in (self.BOS, self.PAD, self.EOS)]
        return " ".join(pieces).replace(" ", "").replace("▁", " ").strip()
