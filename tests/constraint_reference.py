"""qz_constrain_logits' and qz_constraint_advance's rules (include/quantizations.h) restated in numpy on
the raw 16-bit patterns of the logits, and the constructors of qa.TokenAutomaton restated as dense
[S, V] next-state tables built by plain loops: what the kernels, layer_ops' composed routes, the
constructors and the sessions are compared with.  The rounding helpers are the logits-process
reference's.

Row (b, i): s_0 = state[b], s_i = next[s_{i-1}, class_of[tok[b, i]]]; anything out of range makes the
state negative from there on.  Per element: the bias first (x' = round(float32(x) + bias); a NaN logit
keeps its bits; -inf stores -inf), then the masks: a token the state refuses (next < 0 -- `allow` is
not read here) or whose host-mask bit is clear becomes -inf.
"""
import numpy as np

from logits_process_reference import BF16, F16, NEG_INF, from_f32, to_f32  # noqa: F401


# ---- the constructors, dense ---------------------------------------------------------------------
def dense_from_edges(S, V, edges):
    full = np.full((S, V), -1, dtype=np.int64)
    for s, t, n in edges:
        full[s, t] = n
    return full


def dense_from_choices(choices, eos, V):
    """A trie in insertion order (state 0 the root), then the terminal state."""
    child, done = [{}], set()
    for c in choices:
        s = 0
        for t in c:
            if t not in child[s]:
                child.append({})
                child[s][t] = len(child) - 1
            s = child[s][t]
        done.add(s)
    term = len(child)
    full = np.full((term + 1, V), -1, dtype=np.int64)
    for s, kids in enumerate(child):
        for t, n in kids.items():
            full[s, t] = n
    for s in done:
        full[s, eos] = term
    full[term, eos] = term
    return full


def dense_from_byte_dfa(vocab, trans, accepting, eos):
    trans = np.asarray(trans)
    Sb, V = trans.shape[0], len(vocab)
    full = np.full((Sb + 1, V), -1, dtype=np.int64)
    for s in range(Sb):
        for t, w in enumerate(vocab):
            if len(w) == 0:
                continue
            cur = s
            for byte in bytes(w):
                cur = int(trans[cur, byte])
                if cur < 0:
                    break
            full[s, t] = cur if cur >= 0 else -1
        full[s, eos] = Sb if accepting[s] else -1
    full[Sb, eos] = Sb
    return full


def dense_of(class_of, nxt):
    """The [S, V] table a compressed pair stands for."""
    return np.asarray(nxt)[:, np.asarray(class_of).astype(np.int64)]


# ---- the launches --------------------------------------------------------------------------------
def _step(s, t, class_of, nxt, V):
    S = nxt.shape[0]
    if not (0 <= s < S and 0 <= t < V):
        return -1
    n = int(nxt[s, int(class_of[t])])
    return n if 0 <= n < S else -1


def row_states(state, tok, class_of, nxt, V, B, T):
    """int [B, T]: the state of every row, -1 where the automaton leaves the row alone."""
    out = np.full((B, T), -1, dtype=np.int64)
    S = nxt.shape[0]
    for b in range(B):
        s = int(state[b])
        s = s if 0 <= s < S else -1
        out[b, 0] = s
        for i in range(1, T):
            s = _step(s, int(tok[b][i]), class_of, nxt, V) if s >= 0 else -1
            out[b, i] = s
    return out


def constrain(bits, dt, V, T=1, *, state=None, tok=None, class_of=None, nxt=None, mask=None, bias_ids=None,
              bias_vals=None, bias_n=None):
    """bits uint16 [B*T, row]; returns the processed copy (elements past V are never touched)."""
    out = np.array(bits, dtype=np.uint16, copy=True)
    R = out.shape[0]
    B = R // T
    states = None
    if state is not None:
        tk = None if tok is None else np.asarray(tok).reshape(B, T)
        states = row_states(np.asarray(state), tk, np.asarray(class_of), np.asarray(nxt), V, B, T)
    for b in range(B):
        for i in range(T):
            row = out[b * T + i]
            if bias_ids is not None:
                n = min(max(int(bias_n[b]), 0), np.asarray(bias_ids).shape[1])
                ids = np.asarray(bias_ids[b][:n]).astype(np.int64)
                vals = np.asarray(bias_vals[b][:n], dtype=np.float32)
                keep = (ids >= 0) & (ids < V) & ~np.isnan(vals)
                ids, vals = ids[keep], vals[keep]          # distinct by contract
                old = row[ids]
                x = to_f32(old, dt)
                with np.errstate(all="ignore"):
                    y = from_f32((x + vals).astype(np.float32), dt)
                y = np.where(vals == -np.inf, np.uint16(NEG_INF[dt]), y)
                row[ids] = np.where(np.isnan(x), old, y)
            if states is not None and states[b, i] >= 0:
                refused = np.asarray(nxt)[states[b, i], np.asarray(class_of).astype(np.int64)] < 0
                row[:V][refused] = NEG_INF[dt]
            if mask is not None:
                v = np.arange(V)
                words = np.asarray(mask[b]).astype(np.int64) & 0xFFFFFFFF
                row[:V][((words[v >> 5] >> (v & 31)) & 1) == 0] = NEG_INF[dt]
    return out


def advance(state, seq, pos0, pos1, class_of, nxt, V):
    """Returns the new states (int32 [B])."""
    out = np.array(state, dtype=np.int32, copy=True)
    seq = np.asarray(seq)
    B, L = seq.shape
    pos0, pos1 = np.asarray(pos0).reshape(-1), np.asarray(pos1).reshape(-1)
    S = np.asarray(nxt).shape[0]
    for b in range(B):
        lo = max(int(pos0[b if len(pos0) > 1 else 0]) + 1, 0)
        hi = min(int(pos1[b if len(pos1) > 1 else 0]), L - 1)
        s = int(out[b])
        if lo > hi or s < 0:
            continue
        s = s if s < S else -1
        for c in range(lo, hi + 1):
            s = _step(s, int(seq[b, c]), np.asarray(class_of), np.asarray(nxt), V)
            if s < 0:
                break
        out[b] = s if s >= 0 else -2
    return out
