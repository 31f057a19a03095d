"""Host side of the paged KV cache: who holds which page.

The attention launches of csrc/paged_attn.hip read a key through a table: key j of stream b lives in
page ``table[b, j >> 7]`` of a per-layer pool ``[P, Hkv, 128, D]`` at slot ``j & 127``.  One table serves
every layer, so one ``KVPagePool`` serves a whole model.  It owns the device table, a free list, a
refcount per page, each row's page list on the host and the prefix registry.  It is plain Python and
torch, and works with ``device="cpu"``.

Reservation, not growth.  ``reserve(b, n_slots)`` makes row b long enough for n_slots positions, or
raises ``KVPagesExhausted`` and changes nothing.  A caller reserves up to a stream's limit before it
runs, so a captured step never needs a page it does not have and there is no allocator on the device.
This is a library, not a scheduler: whoever gets ``KVPagesExhausted`` waits or releases something.

Every row always names at least one page that nobody else names.  ``release(b)`` gives the row's pages
back and leaves it one private page at entry 0 and -1 elsewhere; with the row's position reset to 0 a
retired row of a captured batch keeps computing on finite data of its own and can never write into a
page that has been handed on.  Hence ``num_pages >= batch``, and every call that would leave some row
unable to get its private page back is refused with ``KVPagesExhausted``.

The invariant the kernels rely on.  A stream only ever writes at positions >= its current position,
and only pages that lie wholly below a position that was final when they were published are ever
shared: the full pages of a prompt after its prefill (``register``), the pages below ``pos >> 7`` of a
stream at position pos (``fork``).  Both entry points assert it.  A shared page is therefore never
written again, by anyone.

Prefix registry.  A dict keyed by ``(salt, id of the previous page's entry, the 128 token ids as
bytes)``: the key is the tokens themselves, no hash is trusted, and because it is a chain an equal
second page under a different first page is no hit.  Entry ids are never reused, so a child of an
evicted page can never be reached through a later page that happens to get the same number.
Registered pages that nobody names stay resident and are evicted least-recently-used, and only when
the free list is empty; a page with a positive refcount is never evicted.
"""
from __future__ import annotations

import copy
from array import array
from collections import OrderedDict

import torch

PAGE = 128  # positions per page: qz_kv_page_size(), the decode head's key chunk


class KVPagesExhausted(RuntimeError):
    """The pool cannot supply the pages a call needs; nothing was changed."""


def _ids(tokens) -> list:
    if isinstance(tokens, torch.Tensor):
        return [int(x) for x in tokens.reshape(-1).tolist()]
    return [int(x) for x in tokens]


class KVPagePool:
    def __init__(self, num_pages: int, batch: int, pages_per_stream: int, device="cpu"):
        if batch < 1 or pages_per_stream < 1:
            raise ValueError("KVPagePool: batch and pages_per_stream must be positive")
        if num_pages < batch:
            raise ValueError("KVPagePool: every row keeps one private page, so num_pages >= batch")
        self.num_pages, self.batch, self.pages_per_stream = int(num_pages), int(batch), int(pages_per_stream)
        self.table = torch.full((batch, pages_per_stream), -1, dtype=torch.int32, device=device)
        self._ref = [0] * num_pages
        self._free = list(range(num_pages - 1, -1, -1))      # a stack: page 0 goes out first
        self._rows = [[] for _ in range(batch)]
        self._entries = {}                                    # key -> (page, entry id)
        self._key_of = {}                                     # registered page -> its key
        self._idle = OrderedDict()                            # registered pages nobody names, oldest first
        self._next_id = 1
        for b in range(batch):
            self._rows[b] = [self._take()]
        self._write_rows(range(batch))

    # ---- inspection
    def pages(self, b: int) -> list:
        return list(self._rows[b])

    def refcount(self, page: int) -> int:
        return self._ref[page]

    def capacity(self, b: int) -> int:
        """Positions row b can hold with the pages it names."""
        return PAGE * len(self._rows[b])

    def stats(self) -> dict:
        held = sum(1 for r in self._ref if r > 0)
        return {"free": len(self._free), "held": held, "idle": len(self._idle), "total": self.num_pages}

    def check(self) -> None:
        """The bookkeeping's own invariants (the tests call it after every step)."""
        named = [0] * self.num_pages
        for row in self._rows:
            assert 1 <= len(row) <= self.pages_per_stream and len(set(row)) == len(row), row
            for p in row:
                named[p] += 1
        assert named == self._ref, (named, self._ref)
        s = self.stats()
        assert s["free"] + s["held"] + s["idle"] == s["total"], s
        assert len(set(self._free)) == len(self._free)
        for p in self._free:
            assert named[p] == 0 and p not in self._key_of, p
        for p in self._idle:
            assert named[p] == 0 and p in self._key_of, p
        for key, (p, _) in self._entries.items():
            assert self._key_of.get(p) == key
        assert len(self._entries) == len(self._key_of)
        assert self._spare_short() <= 0
        want = torch.full((self.batch, self.pages_per_stream), -1, dtype=torch.int32)
        for b, row in enumerate(self._rows):
            want[b, :len(row)] = torch.tensor(row, dtype=torch.int32)
        assert torch.equal(self.table.cpu(), want)

    # ---- internals
    def _take(self) -> int:
        """A page nobody names: from the free list, else the least recently used idle page."""
        if self._free:
            p = self._free.pop()
        elif self._idle:
            p, _ = self._idle.popitem(last=False)
            del self._entries[self._key_of.pop(p)]
        else:
            raise KVPagesExhausted("no free or idle page")
        self._ref[p] = 1
        return p

    def _hold(self, p: int) -> None:
        if self._ref[p] == 0:
            del self._idle[p]            # a free page is never shared: it must be an idle registered one
        self._ref[p] += 1

    def _drop(self, p: int) -> None:
        self._ref[p] -= 1
        if self._ref[p] == 0:
            if p in self._key_of:
                self._idle[p] = None     # most recently used
            else:
                self._free.append(p)

    def _spare_short(self) -> int:
        """Rows that name no page of their own, less the pages that could give them one."""
        need = sum(1 for row in self._rows if not any(self._ref[p] == 1 for p in row))
        return need - len(self._free) - len(self._idle)

    def _write_rows(self, rows) -> None:
        for b in rows:
            row = self._rows[b]
            host = torch.tensor(row + [-1] * (self.pages_per_stream - len(row)), dtype=torch.int32)
            self.table[b].copy_(host)    # one small copy per changed row

    def _transaction(self, fn, rows):
        """Run fn on the bookkeeping; on KVPagesExhausted, or if some row could no longer get a private
        page back, restore every structure and raise.  The device table is written on success only."""
        saved = (copy.deepcopy(self._rows), list(self._ref), list(self._free), dict(self._entries),
                 dict(self._key_of), OrderedDict(self._idle), self._next_id)
        try:
            out = fn()
            if self._spare_short() > 0:
                raise KVPagesExhausted("the call would leave a row without a private page to fall back on")
        except KVPagesExhausted:
            (self._rows, self._ref, self._free, self._entries, self._key_of, self._idle, self._next_id) = saved
            raise
        self._write_rows(rows)
        return out

    def _release(self, b: int) -> None:
        row = self._rows[b]
        keep = next((p for p in row if self._ref[p] == 1 and p not in self._key_of), None)
        for p in row:
            if p != keep:
                self._drop(p)
        self._rows[b] = [keep if keep is not None else self._take()]

    # ---- reservation
    def reserve(self, b: int, n_slots: int) -> None:
        """Make row b hold n_slots positions: ceil(n_slots / 128) pages, the ones it already names
        (shared ones included) counted.  Raises KVPagesExhausted, changing nothing, if the pool cannot
        supply the rest."""
        want = -(-int(n_slots) // PAGE)
        if want > self.pages_per_stream:
            raise ValueError(f"reserve: {n_slots} slots exceed {self.pages_per_stream} pages per stream")

        def fn():
            while len(self._rows[b]) < want:
                self._rows[b].append(self._take())
        if want > len(self._rows[b]):
            self._transaction(fn, [b])

    def release(self, b: int) -> None:
        """Give row b's pages back (refcount - 1 each) and leave it one private page at entry 0."""
        self._transaction(lambda: self._release(b), [b])

    def share(self, b: int, pages) -> None:
        """Map resident pages (a lookup's result) to the front of row b, which must be in the
        released state; its private page follows them."""
        pages = list(pages)
        if len(self._rows[b]) != 1 or self._ref[self._rows[b][0]] != 1 or self._rows[b][0] in self._key_of:
            raise ValueError("share: the row must be released first")
        if len(pages) + 1 > self.pages_per_stream:
            raise ValueError("share: no room for a page of the row's own")
        for p in pages:
            assert p in self._key_of, "only published pages are shared"

        def fn():
            for p in pages:
                self._hold(p)
            self._rows[b] = pages + self._rows[b]
        if pages:
            self._transaction(fn, [b])

    def assign(self, b: int, shared, n_slots: int) -> None:
        """Row b starts over, in one step: release it, map the resident pages `shared` (a lookup's
        result) to its front and reserve up to n_slots positions.  Raises KVPagesExhausted, leaving
        row b's pages and everything else as they were, if the pool cannot supply the rest."""
        shared = list(shared)
        want = -(-int(n_slots) // PAGE)
        if want > self.pages_per_stream or len(shared) + 1 > self.pages_per_stream:
            raise ValueError(f"assign: {n_slots} slots exceed {self.pages_per_stream} pages per stream")
        for p in shared:
            assert p in self._key_of, "only published pages are shared"

        def fn():
            for p in shared:
                self._hold(p)            # before the release, which may evict an idle page
            self._release(b)
            self._rows[b] = shared + self._rows[b]
            while len(self._rows[b]) < want:
                self._rows[b].append(self._take())
        self._transaction(fn, [b])

    def fork(self, src: int, dst: int, pos: int, n_slots: int = 0):
        """Row dst becomes a continuation of row src at position pos (src's current position): dst is
        released, then names src's pages below pos >> 7 (final: src only writes at >= pos) followed by
        its own private page for entry pos >> 7, and is reserved up to n_slots positions -- all or
        nothing.  Returns (src_page, dst_page) when pos & 127 != 0 -- the caller copies that partial
        page, every layer, K and V -- and None otherwise."""
        if src == dst:
            raise ValueError("fork: src and dst must differ")
        n = int(pos) >> 7
        if not 0 <= pos < PAGE * self.pages_per_stream:
            raise ValueError("fork: position outside the stream's table")
        srow = self._rows[src]
        assert n <= len(srow) and (pos & (PAGE - 1) == 0 or n < len(srow)), "src does not hold its own position"
        shared = srow[:n]    # wholly below pos: never written again
        want = -(-int(n_slots) // PAGE)
        if want > self.pages_per_stream:
            raise ValueError(f"fork: {n_slots} slots exceed {self.pages_per_stream} pages per stream")

        def fn():
            for p in shared:
                self._hold(p)
            self._release(dst)
            self._rows[dst] = shared + self._rows[dst]
            while len(self._rows[dst]) < want:
                self._rows[dst].append(self._take())
        self._transaction(fn, [dst])
        return (srow[n], self._rows[dst][n]) if pos & (PAGE - 1) else None

    # ---- prefix registry
    def _chain(self, ids, n_pages, salt):
        parent = 0
        for c in range(n_pages):
            key = (salt, parent, array("q", ids[PAGE * c:PAGE * (c + 1)]).tobytes())
            yield c, key                   # register may add the entry before the chain goes on
            ent = self._entries.get(key)
            if ent is None:
                return
            parent = ent[1]

    def register(self, b: int, tokens, n_full_pages: int, salt=None, final_below=None) -> int:
        """Publish row b's first n_full_pages pages as holding tokens[:128 n_full_pages].  They must be
        full and final: wholly below len(tokens), and below final_below (the row's current position)
        when given.  A page whose content is already published under another page stays private.
        Returns the number of pages newly published."""
        ids = _ids(tokens)
        n = int(n_full_pages)
        assert 0 <= PAGE * n <= len(ids), "only full pages are published"
        assert final_below is None or PAGE * n <= final_below, "only pages below the row's position are final"
        assert n <= len(self._rows[b]), "the row does not hold these pages"
        new = 0
        for c, key in self._chain(ids, n, salt):
            if key not in self._entries:
                p = self._rows[b][c]
                if p in self._key_of:       # published already under another chain (a shared page)
                    break
                self._entries[key] = (p, self._next_id)
                self._key_of[p] = key
                self._next_id += 1
                new += 1
        return new

    def lookup(self, tokens, salt=None) -> list:
        """The longest chain of resident pages that holds a prefix of tokens, at most
        (len(tokens) - 1) // 128 pages: the last prompt token must still run, to give logits."""
        ids = _ids(tokens)
        out = []
        for c, key in self._chain(ids, max(0, (len(ids) - 1) // PAGE), salt):
            ent = self._entries.get(key)
            if ent is None:
                break
            out.append(ent[0])
            if ent[0] in self._idle:
                self._idle.move_to_end(ent[0])
        return out
