"""Shared by the paged attention tests: pools with a NaN page and sentinel pages inside guard bands,
tables built from the positions a case uses, and the gather / scatter that turns a paged call into the
contiguous call it must equal bit for bit.  Plain torch; importing it needs no GPU.

Layout of a case: B = 3 streams, NP = 3 table entries, P = 8 pages.  Streams 0 and 1 name page 0 at
entry 0.  Page 7 is NaN and every entry above a row's needed range names it, so a dependence on an
entry that must not be read shows by value.  Pages no table names hold the sentinel pattern."""
import torch

import footprint as fp

PAGE = 128
B, NP, P = 3, 3, 8
NAN_PAGE = 7
SCRAMBLED = [5, 2, 6, 1, 4, 3]      # private pages, handed out in this order


def build_table(last_pos, overrides=None, table_row=NP):
    """int32 [B, table_row]: stream b gets entries 0 .. last_pos[b] >> 7 (last_pos[b] < 0: none), page 0
    first for streams 0 and 1; everything else names the NaN page.  overrides: {(b, c): entry}."""
    free = list(SCRAMBLED)
    t = torch.full((B, table_row), NAN_PAGE, dtype=torch.int32)
    for b, lp in enumerate(last_pos):
        for c in range(0 if lp < 0 else min(lp >> 7, NP - 1) + 1):
            t[b, c] = 0 if (c == 0 and b < 2) else free.pop(0)
    for (b, c), e in (overrides or {}).items():
        t[b, c] = e
    return t, free          # free: the pages no table names


def make_pools(dt, Hkv, D, unnamed, seed, device):
    """(k_pool, v_pool) [P, Hkv, 128, D] as guarded views (guards of at least one page, poisoned)."""
    out = []
    for s in (seed, seed + 1):
        g = torch.Generator().manual_seed(s)
        pool = torch.randn((P, Hkv, PAGE, D), generator=g).to(dt)
        pool[NAN_PAGE] = float("nan")
        for p in unnamed:
            pool[p] = fp.filled((Hkv, PAGE, D), dt, "sentinel")
        v = fp.guarded(pool.to(device), fill="poison", name="pool")
        assert fp.guard_bytes(D, 2) >= Hkv * PAGE * D * 2, "the guards hold at least one page"
        assert v.is_contiguous() and v.data_ptr() % 16 == 0
        out.append(v)
    return out


def gather(pool, table):
    """The contiguous cache [B, Hkv, 128 NP, D] the table names (an entry outside [0, P): the NaN page)."""
    t = table[:, :NP].to(pool.device).long()
    t = torch.where((t >= 0) & (t < pool.shape[0]), t, torch.full_like(t, NAN_PAGE))
    pages = pool[t]                                     # [B, NP, Hkv, 128, D]
    return pages.permute(0, 2, 1, 3, 4).reshape(t.shape[0], pool.shape[1], NP * PAGE, pool.shape[3]).contiguous()


def scatter(pool_before, cache_before, cache_after, table, written, skipped=None):
    """The pool a paged call must leave: pool_before with the slots `written` ({b: positions}) taken from
    the contiguous call's cache; the contiguous call changed nothing else but the slots `skipped`, which
    the paged call must leave alone (their table entry is invalid)."""
    want = pool_before.clone()
    ch = fp.bits(cache_before) != fp.bits(cache_after)
    for b, slots in written.items():
        for j in slots:
            want[int(table[b, j >> 7]), :, j & (PAGE - 1)] = cache_after[b, :, j]
            ch[b, :, j] = False
    for b, slots in (skipped or {}).items():
        for j in slots:
            ch[b, :, j] = False
    assert not bool(ch.any()), "the contiguous reference wrote outside the window"
    return want


def operands(dt, Hq, Hkv, D, T, seed, device):
    """q [B, T, Hq D], k / v [B, T, Hkv D], cos / sin [B, T, D]."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((B, T, Hq * D), generator=g).to(dt).to(device)
    k = torch.randn((B, T, Hkv * D), generator=g).to(dt).to(device)
    v = torch.randn((B, T, Hkv * D), generator=g).to(dt).to(device)
    ang = torch.rand((B, T, D // 2), generator=g) * 6.0
    cos = torch.cat((ang.cos(), ang.cos()), -1).to(dt).to(device)
    sin = torch.cat((ang.sin(), ang.sin()), -1).to(dt).to(device)
    return q, k, v, cos, sin
