"""CPU: the host side of the paged KV cache (quantizations_amd/kv_pages.py) on device "cpu" --
reservation counts and the all-or-nothing failure, release, the chained prefix registry, LRU eviction
of idle pages only, fork bookkeeping, and a randomised sequence that checks the bookkeeping's
invariants (KVPagePool.check plus the counts restated here) after every call."""
import random

import pytest
import torch

from quantizations_amd.kv_pages import PAGE, KVPagePool, KVPagesExhausted


def snapshot(pool):
    return (pool.table.clone(), [pool.refcount(p) for p in range(pool.num_pages)], list(pool._free),
            [pool.pages(b) for b in range(pool.batch)], dict(pool._entries), list(pool._idle))


def same(a, b):
    return torch.equal(a[0], b[0]) and a[1:] == b[1:]


def invariants(pool):
    pool.check()
    named = {}
    for b in range(pool.batch):
        for p in pool.pages(b):
            named[p] = named.get(p, 0) + 1
    for p in range(pool.num_pages):
        assert pool.refcount(p) == named.get(p, 0)
    s = pool.stats()
    assert s["free"] + s["held"] + s["idle"] == s["total"] == pool.num_pages
    assert not set(pool._free) & set(named)


def test_page_size_matches_the_library():
    from quantizations_amd import _lib, layer_ops
    assert _lib.lib.qz_kv_page_size() == PAGE == layer_ops.KV_PAGE == layer_ops.ATTN_CHUNK == 128


def test_every_row_starts_with_one_private_page():
    pool = KVPagePool(6, 3, 4)
    assert pool.table.dtype == torch.int32 and tuple(pool.table.shape) == (3, 4)
    firsts = [pool.pages(b) for b in range(3)]
    assert all(len(r) == 1 for r in firsts) and len({r[0] for r in firsts}) == 3
    assert pool.table[:, 1:].eq(-1).all() and pool.table[:, 0].tolist() == [r[0] for r in firsts]
    assert pool.stats() == {"free": 3, "held": 3, "idle": 0, "total": 6}
    with pytest.raises(ValueError):
        KVPagePool(2, 3, 4)
    invariants(pool)


@pytest.mark.parametrize("slots, pages", [(1, 1), (127, 1), (128, 1), (129, 2), (256, 2), (257, 3), (512, 4)])
def test_reserve_takes_the_ceiling(slots, pages):
    pool = KVPagePool(8, 2, 4)
    pool.reserve(0, slots)
    assert len(pool.pages(0)) == pages and pool.capacity(0) == 128 * pages
    assert pool.table[0, :pages].tolist() == pool.pages(0) and pool.table[0, pages:].eq(-1).all()
    assert len(pool.pages(1)) == 1
    pool.reserve(0, 1)      # never shrinks
    assert len(pool.pages(0)) == pages
    invariants(pool)
    with pytest.raises(ValueError):
        pool.reserve(0, 513)


def test_exhaustion_changes_nothing():
    pool = KVPagePool(5, 2, 4)
    pool.reserve(0, 300)            # 3 pages: 1 free left
    before = snapshot(pool)
    with pytest.raises(KVPagesExhausted):
        pool.reserve(1, 384)        # wants 2 more
    assert same(before, snapshot(pool))
    assert issubclass(KVPagesExhausted, RuntimeError)
    pool.reserve(1, 256)            # one more is there
    invariants(pool)
    assert pool.stats()["free"] == 0


def test_release_leaves_one_private_page_and_frees_only_its_own():
    pool = KVPagePool(8, 3, 4)
    toks = list(range(300))
    pool.reserve(0, 300)
    pool.register(0, toks, 2)
    shared = pool.lookup(toks)
    assert shared == pool.pages(0)[:2]
    pool.share(1, shared)
    pool.reserve(1, 300)
    assert pool.pages(1)[:2] == shared and [pool.refcount(p) for p in shared] == [2, 2]
    pool.release(0)
    assert len(pool.pages(0)) == 1 and pool.refcount(pool.pages(0)[0]) == 1
    assert pool.table[0, 1:].eq(-1).all() and pool.table[0, 0].item() == pool.pages(0)[0]
    assert [pool.refcount(p) for p in shared] == [1, 1]        # row 1 still holds them
    assert pool.pages(0)[0] not in pool.pages(1)
    assert not set(pool._free) & set(pool.pages(1))
    invariants(pool)
    pool.release(1)
    assert [pool.refcount(p) for p in shared] == [0, 0] and pool.stats()["idle"] == 2
    invariants(pool)


def test_lookup_is_chained_salted_and_leaves_the_last_token():
    pool = KVPagePool(12, 3, 4)
    first, second = list(range(1000, 1128)), list(range(2000, 2128))
    other = list(range(3000, 3128))
    pool.reserve(0, 384)
    pool.register(0, first + second + [7] * 100, 2)
    # an equal second page under a different first page is no hit, nor is the second page alone
    assert pool.lookup(other + second + [1]) == []
    assert pool.lookup(second + [1]) == []
    assert pool.lookup(first + second + [1]) == pool.pages(0)[:2]
    assert pool.lookup(first + other + [1]) == pool.pages(0)[:1]
    # a different salt shares nothing, in either direction
    assert pool.lookup(first + second + [1], salt="adapter-1") == []
    pool.reserve(1, 384)
    pool.register(1, first + second + [1], 2, salt="adapter-1")
    assert pool.lookup(first + second + [1], salt="adapter-1") == pool.pages(1)[:2]
    assert pool.lookup(first + second + [1]) == pool.pages(0)[:2]
    # at most (S - 1) // 128 pages: the last prompt token must still run
    for S, want in [(1, 0), (128, 0), (129, 1), (256, 1), (257, 2), (300, 2)]:
        got = pool.lookup((first + second + [7] * 100)[:S])
        assert len(got) == want == min(2, (S - 1) // 128), (S, got)
    assert pool.lookup(torch.tensor(first + second + [1])) == pool.pages(0)[:2]
    invariants(pool)


def test_register_asserts_the_pages_are_full_and_final():
    pool = KVPagePool(6, 2, 4)
    pool.reserve(0, 300)
    with pytest.raises(AssertionError):
        pool.register(0, list(range(200)), 2)                    # the second page is not full
    with pytest.raises(AssertionError):
        pool.register(0, list(range(300)), 2, final_below=200)   # not below the row's position
    assert pool.register(0, list(range(300)), 2, final_below=300) == 2
    assert pool.register(0, list(range(300)), 2) == 0            # already there
    invariants(pool)


def test_eviction_takes_idle_pages_only_lru_and_only_when_nothing_is_free():
    pool = KVPagePool(6, 2, 4)
    a, b = [1] * 128, [2] * 128
    pool.reserve(0, 257)
    pool.register(0, a + b + [0], 2)
    pa, pb = pool.pages(0)[:2]
    pool.release(0)                                   # a, b idle; row 0 keeps its third page
    assert pool.stats() == {"free": 2, "held": 2, "idle": 2, "total": 6}
    pool.reserve(1, 384)                              # takes the 2 free pages: no eviction yet
    assert pool.stats() == {"free": 0, "held": 4, "idle": 2, "total": 6}
    assert pool.lookup(a + b + [0]) == [pa, pb]
    pool.lookup(a + [0])                              # touches a: b is now the least recently used
    pool.reserve(0, 129)                              # free list empty: evicts b
    assert pool.pages(0)[1] == pb and pool.lookup(a + b + [0]) == [pa]
    # a page somebody names survives any pressure
    pool.release(0)
    pool.share(0, [pa])
    assert pool.refcount(pa) == 1 and pool.stats()["idle"] == 0
    before = snapshot(pool)
    pool.reserve(0, 384)                              # the page released above is free again
    with pytest.raises(KVPagesExhausted):
        pool.reserve(1, 512)
    assert pool.pages(0)[0] == pa and pool.lookup(a + [0]) == [pa]
    assert before[1][pa] == 1
    invariants(pool)


def test_fork_shares_full_pages_and_copies_the_partial_one():
    pool = KVPagePool(10, 3, 4)
    pool.reserve(0, 400)
    src = pool.pages(0)
    copy_pair = pool.fork(0, 1, 300)                  # pos >> 7 = 2, pos & 127 = 44
    assert pool.pages(1)[:2] == src[:2] and len(pool.pages(1)) == 3
    assert copy_pair == (src[2], pool.pages(1)[2]) and pool.pages(1)[2] not in src
    assert [pool.refcount(p) for p in src] == [2, 2, 1, 1] and pool.refcount(pool.pages(1)[2]) == 1
    assert pool.table[1].tolist() == pool.pages(1) + [-1]
    invariants(pool)
    assert pool.fork(0, 2, 256) is None               # on a page edge: nothing to copy
    assert pool.pages(2)[:2] == src[:2] and len(pool.pages(2)) == 3 and pool.refcount(pool.pages(2)[2]) == 1
    assert [pool.refcount(p) for p in src[:2]] == [3, 3]
    invariants(pool)
    pool.fork(0, 1, 100)                              # dst is released first; below one page nothing is shared
    assert len(pool.pages(1)) == 1 and pool.pages(1)[0] not in src
    assert [pool.refcount(p) for p in src[:2]] == [2, 2]
    invariants(pool)
    with pytest.raises(ValueError):
        pool.fork(0, 0, 10)
    with pytest.raises(ValueError):
        pool.fork(0, 1, 512)


def test_a_call_that_would_strand_a_row_is_refused():
    """Row 0's only page is shared with row 1, so row 0 needs a free page to fall back on when it is released:
    the reservation that would take the last one is refused, although a page is free."""
    pool = KVPagePool(4, 2, 4)
    pool.register(0, [5] * 128, 1)
    pool.share(1, pool.lookup([5] * 129))
    assert pool.pages(1)[0] == pool.pages(0)[0] and pool.refcount(pool.pages(0)[0]) == 2 and len(pool.pages(0)) == 1
    pool.reserve(1, 384)            # takes one of the two free pages
    before = snapshot(pool)
    assert pool.stats()["free"] == 1
    with pytest.raises(KVPagesExhausted):
        pool.reserve(1, 512)        # the last free page is row 0's way back to a private page
    assert same(before, snapshot(pool))
    pool.release(0)
    assert pool.refcount(pool.pages(0)[0]) == 1 and pool.pages(0)[0] not in pool.pages(1)
    pool.release(1)
    invariants(pool)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_sequences_keep_the_books(seed):
    rng = random.Random(seed)
    B, NP = 4, 4
    pool = KVPagePool(11, B, NP)
    pos = [0] * B
    prompts = [[rng.randrange(3) for _ in range(128)] for _ in range(3)]
    refused = 0
    for _ in range(400):
        op = rng.choice(["reserve", "release", "fork", "admit", "lookup"])
        b = rng.randrange(B)
        before = snapshot(pool)
        try:
            if op == "reserve":
                n = rng.randrange(1, 128 * NP + 1)
                pool.reserve(b, n)
                assert pool.capacity(b) >= n
            elif op == "release":
                pool.release(b)
                pos[b] = 0
                assert len(pool.pages(b)) == 1
            elif op == "fork":
                d = rng.randrange(B)
                if d != b and pool.capacity(b) > 0:
                    p = rng.randrange(pool.capacity(b))
                    pair = pool.fork(b, d, p)
                    pos[d] = p
                    assert (pair is None) == (p % 128 == 0)
                    assert pool.pages(d)[:p >> 7] == pool.pages(b)[:p >> 7]
            elif op == "admit":
                toks = sum((prompts[rng.randrange(3)] for _ in range(rng.randrange(1, NP))), []) + [9] * rng.randrange(1, 100)
                pool.release(b)
                hit = pool.lookup(toks)
                assert len(hit) <= (len(toks) - 1) // 128
                try:
                    pool.share(b, hit)
                    pool.reserve(b, len(toks))
                except KVPagesExhausted:
                    pool.release(b)
                    raise
                pool.register(b, toks, len(toks) // 128, final_below=len(toks))
                pos[b] = len(toks)
            else:
                toks = prompts[rng.randrange(3)] + prompts[rng.randrange(3)] + [1]
                for p in pool.lookup(toks):
                    assert p in pool._key_of
        except KVPagesExhausted:
            refused += 1
            if op in ("reserve", "fork"):
                assert same(before, snapshot(pool))
        invariants(pool)
    print("refused", refused)
