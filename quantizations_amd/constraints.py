"""Token-level automata for constrained decoding (qa.TokenAutomaton), in the compressed form the
captured step reads on the device (include/quantizations.h, qz_constrain_logits):

  class_of  int16 [V]              token -> equivalence class; tokens with identical transition
                                   columns share a class
  next      int32 [S, C]           next state, -1 = refused
  allow     int32 [S, ceil(C/32)]  bit c & 31 of word c >> 5 is set iff next[s, c] >= 0

Everything here is host-side numpy; `.to(device)` hands the three tables out as tensors.  A stream's
state is an int32 on the device: a state of the table, -1 for "unconstrained by request", -2 once a
refused transition was taken.  Regex and JSON-schema compilers are out of scope: `from_byte_dfa` takes
the byte-level DFA such a compiler produces and a tokenizer's vocabulary.
"""
from __future__ import annotations

import math
from typing import Iterable, List, Sequence, Tuple

import numpy as np
import torch

MAX_CLASSES = 32767      # class_of is int16
MAX_STATES = 2 ** 31 - 1  # states are int32


def _allow_bits(nxt: np.ndarray) -> np.ndarray:
    S, C = nxt.shape
    W = (C + 31) // 32
    ok = np.zeros((S, W * 32), dtype=np.uint32)
    ok[:, :C] = nxt >= 0
    words = (ok.reshape(S, W, 32) << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint64)
    return words.astype(np.uint32).view(np.int32)


class TokenAutomaton:
    """A deterministic automaton over token ids: state s allows token t iff next[s, class_of[t]] >= 0,
    and taking it leads there.  `starts` are the states streams may be opened in (constraint_start);
    construction refuses a table in which some state reachable from a start allows no token, since a
    stream arriving there could pick nothing."""

    def __init__(self, class_of, next, starts: Sequence[int] = (0,)):
        class_of = np.ascontiguousarray(class_of)
        nxt = np.ascontiguousarray(next)
        if class_of.ndim != 1 or nxt.ndim != 2:
            raise ValueError("TokenAutomaton: class_of must be [V] and next [S, C]")
        S, C = nxt.shape
        if C > MAX_CLASSES or S > MAX_STATES:
            raise ValueError(f"TokenAutomaton: {C} token classes and {S} states; at most {MAX_CLASSES} classes "
                             f"(int16) and {MAX_STATES} states (int32) fit the device tables")
        if S < 1 or C < 1 or class_of.size < 1:
            raise ValueError("TokenAutomaton: at least one state, one class and one token")
        if class_of.min() < 0 or class_of.max() >= C:
            raise ValueError("TokenAutomaton: class_of holds a class outside [0, C)")
        if nxt.max() >= S:
            raise ValueError("TokenAutomaton: next holds a state outside [0, S)")
        self.class_of = class_of.astype(np.int16)
        self.next = np.where(nxt < 0, -1, nxt).astype(np.int32)
        self.allow = _allow_bits(self.next)
        self.starts = tuple(int(s) for s in starts)
        if any(not 0 <= s < S for s in self.starts):
            raise ValueError(f"TokenAutomaton: a start state outside [0, {S})")
        self._check_no_dead_end()

    V = property(lambda self: int(self.class_of.shape[0]))
    S = property(lambda self: int(self.next.shape[0]))
    C = property(lambda self: int(self.next.shape[1]))

    def _check_no_dead_end(self) -> None:
        # classes no token belongs to cannot be taken: they do not count as a way out
        used = np.zeros(self.C, dtype=bool)
        used[self.class_of] = True
        live = (self.next >= 0) & used[None, :]
        seen = np.zeros(self.S, dtype=bool)
        todo = list(set(self.starts))
        seen[todo] = True
        while todo:
            s = todo.pop()
            if not live[s].any():
                raise ValueError(f"TokenAutomaton: state {s} is reachable from a start state and allows no token")
            for n in np.unique(self.next[s][live[s]]):
                if not seen[n]:
                    seen[n] = True
                    todo.append(int(n))

    # ---- constructors ------------------------------------------------------------------------
    @classmethod
    def from_dense(cls, next_full, starts: Sequence[int] = (0,)) -> "TokenAutomaton":
        """next_full [S, V]: the next state of every (state, token), negative = refused."""
        full = np.asarray(next_full)
        if full.ndim != 2 or full.shape[0] < 1 or full.shape[1] < 1:
            raise ValueError("TokenAutomaton.from_dense: next_full must be [S, V]")
        full = np.where(full < 0, -1, full).astype(np.int32)
        cols, inv = np.unique(full, axis=1, return_inverse=True)
        if cols.shape[1] > MAX_CLASSES:
            raise ValueError(f"TokenAutomaton: {cols.shape[1]} token classes and {full.shape[0]} states; at most "
                             f"{MAX_CLASSES} classes (int16) fit the device tables")
        return cls(np.asarray(inv).reshape(-1), cols, starts)

    @classmethod
    def from_edges(cls, S: int, V: int, edges: Iterable[Tuple[int, int, int]],
                   starts: Sequence[int] = (0,)) -> "TokenAutomaton":
        """edges: (state, token, next_state) triples; every other (state, token) is refused."""
        full = np.full((int(S), int(V)), -1, dtype=np.int32)
        for s, t, n in edges:
            if not (0 <= s < S and 0 <= t < V and 0 <= n < S):
                raise ValueError(f"TokenAutomaton.from_edges: edge ({s}, {t}, {n}) outside {S} states x {V} tokens")
            full[s, t] = n
        return cls.from_dense(full, starts)

    @classmethod
    def from_choices(cls, choices: Sequence[Sequence[int]], eos: int, V: int) -> "TokenAutomaton":
        """A trie over token sequences from state 0: after a complete choice only `eos` is allowed, and
        it leads to a terminal state that again allows only `eos` (a choice that is a prefix of another
        allows `eos` and the other's next token)."""
        choices = [[int(t) for t in c] for c in choices]
        if not choices or any(len(c) == 0 for c in choices):
            raise ValueError("TokenAutomaton.from_choices: at least one choice, none of them empty")
        if not 0 <= int(eos) < V or any(t == eos or not 0 <= t < V for c in choices for t in c):
            raise ValueError("TokenAutomaton.from_choices: eos and the choices' tokens must lie in [0, V), and no "
                             "choice may hold eos")
        child = [{}]
        done = set()
        for c in choices:
            s = 0
            for t in c:
                if t not in child[s]:
                    child.append({})
                    child[s][t] = len(child) - 1
                s = child[s][t]
            done.add(s)
        term = len(child)
        edges = [(s, t, n) for s, kids in enumerate(child) for t, n in kids.items()]
        edges += [(s, int(eos), term) for s in sorted(done)] + [(term, int(eos), term)]
        return cls.from_edges(term + 1, V, edges)

    @classmethod
    def from_byte_dfa(cls, vocab: Sequence[bytes], trans, accepting, eos: int) -> "TokenAutomaton":
        """The token-level product of a byte DFA: trans int32 [Sb, 256] (-1 = dead), accepting bool [Sb],
        vocab one `bytes` per token id (an empty entry: the token is refused everywhere).  Token t leads
        from state s where its bytes lead; accepting states also allow `eos`, which leads to the
        terminal state Sb that allows only `eos`.  State 0 of the DFA is the start."""
        trans = np.asarray(trans, dtype=np.int32)
        accepting = np.asarray(accepting, dtype=bool).reshape(-1)
        V = len(vocab)
        if trans.ndim != 2 or trans.shape[1] != 256 or accepting.shape[0] != trans.shape[0] or trans.shape[0] < 1:
            raise ValueError("TokenAutomaton.from_byte_dfa: trans must be [Sb, 256] and accepting [Sb]")
        if not 0 <= int(eos) < V:
            raise ValueError("TokenAutomaton.from_byte_dfa: eos must be a token of the vocabulary")
        Sb = trans.shape[0]
        lens = np.array([len(w) for w in vocab], dtype=np.int64)
        L = int(lens.max()) if V else 0
        mat = np.zeros((V, max(L, 1)), dtype=np.int64)
        for t, w in enumerate(vocab):
            mat[t, :len(w)] = np.frombuffer(bytes(w), dtype=np.uint8)
        cur = np.repeat(np.arange(Sb, dtype=np.int32)[:, None], V, axis=1)      # [Sb, V]
        for j in range(L):
            step = trans[np.maximum(cur, 0), mat[None, :, j]]
            step = np.where(cur >= 0, step, -1)
            cur = np.where((lens > j)[None, :], step, cur)
        cur[:, lens == 0] = -1
        cur[:, eos] = np.where(accepting, Sb, -1)
        last = np.full((1, V), -1, dtype=np.int32)
        last[0, eos] = Sb
        return cls.from_dense(np.vstack((np.where(cur < 0, -1, cur).astype(np.int32), last)))

    @classmethod
    def concat(cls, automata: Sequence["TokenAutomaton"]) -> Tuple["TokenAutomaton", List[int]]:
        """One table for several grammars over one vocabulary: returns (automaton, starts), starts[k] the
        state automaton k's state 0 became.  A token's joint class is the tuple of its classes; no
        [S, V] table is made."""
        automata = list(automata)
        if not automata or any(a.V != automata[0].V for a in automata):
            raise ValueError("TokenAutomaton.concat: at least one automaton, all over the same vocabulary")
        stack = np.stack([a.class_of for a in automata])                       # [n, V]
        joint, inv = np.unique(stack, axis=1, return_inverse=True)             # [n, Cj], [V]
        if joint.shape[1] > MAX_CLASSES:
            raise ValueError(f"TokenAutomaton: {joint.shape[1]} joint token classes and "
                             f"{sum(a.S for a in automata)} states; at most {MAX_CLASSES} classes (int16) fit")
        offsets = np.cumsum([0] + [a.S for a in automata])
        rows = []
        for k, a in enumerate(automata):
            part = a.next[:, joint[k]]
            rows.append(np.where(part >= 0, part + offsets[k], -1))
        starts = [int(offsets[k] + s) for k, a in enumerate(automata) for s in a.starts[:1]]
        every = [int(offsets[k] + s) for k, a in enumerate(automata) for s in a.starts]
        out = cls(np.asarray(inv).reshape(-1), np.vstack(rows), every)
        return out, starts

    # ---- host-side use -----------------------------------------------------------------------
    def step(self, state: int, token: int) -> int:
        """The state after `token`, or -1 where it is refused (or the state / token is out of range)."""
        if not (0 <= state < self.S and 0 <= token < self.V):
            return -1
        return int(self.next[state, self.class_of[token]])

    def allowed(self, state: int) -> np.ndarray:
        """bool [V]: the tokens `state` allows."""
        return self.next[state, self.class_of] >= 0

    def to(self, device):
        """(class_of int16 [V], next int32 [S, C], allow int32 [S, ceil(C/32)]) as tensors on `device`."""
        return (torch.from_numpy(self.class_of).to(device), torch.from_numpy(self.next).to(device),
                torch.from_numpy(self.allow).to(device))


def bias_row(bias, V: int = None) -> Tuple[List[int], List[float]]:
    """A stream's logit bias ({token id: bias} or (id, bias) pairs) as (ids, values): ids must be
    distinct integers (inside [0, V) when V is given), a bias finite or -inf (a ban)."""
    items = list(bias.items()) if hasattr(bias, "items") else [tuple(p) for p in bias]
    ids, vals = [], []
    for t, v in items:
        if isinstance(t, bool) or int(t) != t:
            raise ValueError(f"logit_bias: token id {t!r} is not an integer")
        v = float(v)
        if math.isnan(v) or v == math.inf:
            raise ValueError(f"logit_bias: the bias of token {int(t)} is {v}; it must be finite or -inf")
        if V is not None and not 0 <= int(t) < V:
            raise ValueError(f"logit_bias: token {int(t)} outside the vocabulary of {V}")
        ids.append(int(t))
        vals.append(v)
    if len(set(ids)) != len(ids):
        raise ValueError("logit_bias: a token id occurs twice")
    return ids, vals
