"""CPU restatement of ctcdecode's CTC prefix beam search (parlance/ctcdecode `DecoderState::next`, `PathTrie`,
`get_pruned_log_probs`, `log_sum_exp`, `prefix_compare`) as CTCBeamDecoder runs it for the reference
(multi_target_lip2speech/sequence_generator.py:20-38: no language model, alpha = beta = 0, cutoff_prob = 1,
log_probs_input = False, blank 0).  ctcdecode is not vendored by the reference: this restatement is UNPINNED (written from
the algorithm, not checked against a build of the wheel), the same status as the unit BeamSearch.step restatement.

numpy float32 scalars throughout, as the C++ is float.  "Minus infinity" is -FLT_MAX.  Prefix identity is the trie's: a
table (parent node, character) -> node whose entries are never deleted, so a prefix pruned from the beam and extended into
again later is the SAME node (get_path_trie revives it) and merges with any beam member that already extends it.  Where
ctcdecode's order is unspecified (nth_element, std::sort on equal keys) the ties are broken by the candidate's slot:
beam member i, then its extensions in top-K order (slot i*(K+1) + 1 + k) - the order the HIP kernel uses.
"""
import struct

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
NEG = np.float32(-FLT_MAX)
FLT_MIN = np.float32(np.finfo(np.float32).tiny)


def lse(x, y):
    """ctcdecode log_sum_exp (float)."""
    x, y = np.float32(x), np.float32(y)
    if x <= NEG:
        return y
    if y <= NEG:
        return x
    m = max(x, y)
    return np.float32(np.log(np.float32(np.exp(np.float32(x - m)) + np.exp(np.float32(y - m)))) + m)


def softmax32(logits):
    """fp32 softmax over the last axis (torch.nn.functional.softmax on CPU)."""
    return __import__("torch").softmax(__import__("torch").from_numpy(np.ascontiguousarray(logits, np.float32)), -1).numpy()


def pruned_log_probs(p, K):
    """get_pruned_log_probs: the K most probable classes (p descending, ties by the smaller class), log(p + FLT_MIN)."""
    p = np.asarray(p, np.float32)
    order = np.argsort(-p, kind="stable")[:K]
    return [(int(c), np.float32(np.log(np.float32(p[c] + FLT_MIN)))) for c in order]


def _ord(f):
    u = struct.unpack("<I", struct.pack("<f", float(np.float32(f))))[0]
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def _key(score, ch, slot):
    """The kernel's sort key (larger = better): score, then the smaller character (root = -1), then the smaller slot."""
    return (_ord(score) << 32) | ((8191 - (ch + 1)) << 13) | (8191 - slot)


class _Member:
    __slots__ = ("node", "par", "ch", "labels", "b", "nb", "sc")

    def __init__(self, node, par, ch, labels, b, nb):
        self.node, self.par, self.ch, self.labels = node, par, ch, labels
        self.b, self.nb = np.float32(b), np.float32(nb)
        self.sc = lse(self.b, self.nb)


def _ext(m, c, lp):
    """log p of the extension m + c (DecoderState::next)."""
    if c == m.ch:
        return np.float32(lp + m.b) if m.b > NEG else NEG
    return np.float32(lp + m.sc)


def beam_search(probs, beam=30, cutoff_top_n=40, blank=0, fresh_ids=False, trace=None):
    """probs [T, V] float32 (softmax output).  Returns the final beam best first: list of (labels tuple, score) with
    score = ctcdecode's beam score (-log p).  fresh_ids=True gives every surviving extension a new node (the WRONG scheme:
    a revived prefix no longer merges - kept to show the test data exercises the revival path).  trace: a list that receives, per
    frame, the best beam + 1 candidates in order as (score, "own" / "ext", log p of the extending class or None, member index): what
    a caller needs to show that every survivor, and the first candidate dropped, is decided by a gap or by an exact tie."""
    probs = np.asarray(probs, np.float32)
    T, V = probs.shape
    K = min(cutoff_top_n, V)
    table = {}
    n_nodes = 1
    cur = [_Member(0, -1, -1, (), 0.0, NEG)]
    for t in range(T):
        topk = pruned_log_probs(probs[t], K)
        rank = {c: k for k, (c, _) in enumerate(topk)}
        kb = rank.get(blank, -1)
        index_of = {m.node: i for i, m in enumerate(cur)}
        merged, own = set(), []
        for m in cur:
            bc = np.float32(topk[kb][1] + m.sc) if kb >= 0 else NEG
            nbc = NEG
            kc = rank.get(m.ch, -1) if m.ch >= 0 else -1
            if kc >= 0:
                nbc = lse(nbc, np.float32(topk[kc][1] + m.nb))
                pi = index_of.get(m.par, -1)
                if pi >= 0:
                    nbc = lse(nbc, _ext(cur[pi], m.ch, topk[kc][1]))
                    merged.add((pi, kc))
            own.append((bc, nbc))
        cands = []
        for i, m in enumerate(cur):
            s = i * (K + 1)
            bc, nbc = own[i]
            cands.append((_key(lse(bc, nbc), m.ch, s), ("own", i, bc, nbc)))
            for k, (c, lp) in enumerate(topk):
                if c == blank or (i, k) in merged:
                    continue
                nbv = _ext(m, c, lp)
                cands.append((_key(nbv, c, s + 1 + k), ("ext", i, c, nbv)))
        cands.sort(key=lambda x: -x[0])
        if trace is not None:
            trace.append([(lse(cd[2], cd[3]), "own", None, cd[1]) if cd[0] == "own" else (cd[3], "ext", rank[cd[2]], cd[1]) for _, cd in cands[:beam + 1]])
        nxt = []
        for _, cand in cands[:beam]:
            if cand[0] == "own":
                _, i, bc, nbc = cand
                m = cur[i]
                nxt.append(_Member(m.node, m.par, m.ch, m.labels, bc, nbc))
            else:
                _, i, c, nbv = cand
                m = cur[i]
                k = (m.node, c)
                if fresh_ids or k not in table:
                    table[k] = n_nodes
                    n_nodes += 1
                nxt.append(_Member(table[k], m.node, c, m.labels + (c,), NEG, nbv))
        cur = nxt
    return [(m.labels, float(-m.sc)) for m in cur]


def exact_prefix_logprobs(probs, blank=0):
    """Brute force: log P(prefix) = log of the summed probability of every alignment that collapses to it (float64)."""
    import itertools
    probs = np.asarray(probs, np.float64)
    T, V = probs.shape
    acc = {}
    for path in itertools.product(range(V), repeat=T):
        p = 1.0
        for t, c in enumerate(path):
            p *= probs[t, c]
        out, prev = [], None
        for c in path:
            if c != prev and c != blank:
                out.append(c)
            prev = c
        acc[tuple(out)] = acc.get(tuple(out), 0.0) + p
    return {k: float(np.log(v)) for k, v in acc.items()}


def greedy_labels(probs):
    """Framewise argmax of the softmax (ties -> first index), blanks and repeats kept."""
    return np.asarray(probs, np.float32).argmax(-1).astype(np.int64)


class _PathTrie:
    """ctcdecode path_trie.{h,cpp}, literally: children in insertion order, exists_, get_path_trie revives a removed child,
    remove() deletes a childless node and then its parent if that is childless and removed too."""

    def __init__(self, parent=None, character=-1):
        self.parent, self.character, self.children = parent, character, []
        self.exists = True
        self.log_prob_b_prev = self.log_prob_nb_prev = NEG
        self.log_prob_b_cur = self.log_prob_nb_cur = NEG
        self.score = NEG

    def get_path_trie(self, c):
        for ch, node in self.children:
            if ch == c:
                if not node.exists:
                    node.exists = True
                    node.log_prob_b_prev = node.log_prob_nb_prev = NEG
                    node.log_prob_b_cur = node.log_prob_nb_cur = NEG
                return node
        node = _PathTrie(self, c)
        self.children.append((c, node))
        return node

    def iterate_to_vec(self, out):
        if self.exists:
            self.log_prob_b_prev, self.log_prob_nb_prev = self.log_prob_b_cur, self.log_prob_nb_cur
            self.log_prob_b_cur = self.log_prob_nb_cur = NEG
            self.score = lse(self.log_prob_b_prev, self.log_prob_nb_prev)
            out.append(self)
        for _, node in self.children:
            node.iterate_to_vec(out)

    def remove(self):
        self.exists = False
        if not self.children:
            self.parent.children = [(c, n) for c, n in self.parent.children if n is not self]
            if not self.parent.children and not self.parent.exists:
                self.parent.remove()

    def labels(self):
        out, n = [], self
        while n.parent is not None:
            out.append(n.character)
            n = n.parent
        return tuple(reversed(out))


def beam_search_trie(probs, beam=30, cutoff_top_n=40, blank=0):
    """DecoderState::next + decode() as ctcdecode writes them (characters outer, prefixes inner, a PathTrie), independent of
    beam_search's member-centric form.  Ties that ctcdecode leaves to nth_element are broken by a stable sort of the trie's
    DFS order; equal (score, character) pairs only occur among prefixes of probability 0."""
    probs = np.asarray(probs, np.float32)
    root = _PathTrie()
    root.score = root.log_prob_b_prev = np.float32(0.0)
    prefixes = [root]
    for t in range(probs.shape[0]):
        for c, lp in pruned_log_probs(probs[t], min(cutoff_top_n, probs.shape[1])):
            for p in prefixes[:beam]:
                if c == blank:
                    p.log_prob_b_cur = lse(p.log_prob_b_cur, np.float32(lp + p.score))
                    continue
                if c == p.character:
                    p.log_prob_nb_cur = lse(p.log_prob_nb_cur, np.float32(lp + p.log_prob_nb_prev))
                new = p.get_path_trie(c)
                log_p = NEG
                if c == p.character and p.log_prob_b_prev > NEG:
                    log_p = np.float32(lp + p.log_prob_b_prev)
                elif c != p.character:
                    log_p = np.float32(lp + p.score)
                new.log_prob_nb_cur = lse(new.log_prob_nb_cur, log_p)
        prefixes = []
        root.iterate_to_vec(prefixes)
        prefixes.sort(key=lambda n: (-float(n.score), n.character))   # prefix_compare
        for p in prefixes[beam:]:
            p.remove()
        prefixes = prefixes[:beam]
    return [(p.labels(), float(-p.score)) for p in prefixes]
