"""Decoding a model whose linears are Linear4bit at the speed of the benchmark's loop: the fused
single-GPU layout (prepare_for_decode), a decode step captured once into a HIP graph together with
its token pick and feedback (DecodeSession), and generate() on top of both.

The pick is layer_ops.sample_step -- per-stream temperature, top-k and top-p read on the device, so
a replay follows set_sampling() -- or layer_ops.greedy_step when every stream is greedy at capture.
DecodeSession / generate() take equal-length prompts and move every stream together; StreamSession
/ generate_ragged() keep a position per stream on the device (prompts of different lengths, a
finished stream's row handed to the next prompt without recapturing).  SpeculativeSession /
prompt_lookup_num_tokens= verify prompt-lookup drafts: several tokens per stream and step, the
same tokens in fewer reads of the weights -- greedy, or with sample=True / prompt_lookup_sampling=True
the tokens each position's uniform number draws.  set_penalties() / repetition_penalty=,
presence_penalty=, frequency_penalty=, no_repeat_ngram_size=, min_new_tokens= put
layer_ops.process_logits in front of every pick, inside the captured step: the processors read each
stream's history and their own parameters on the device.  constraint= (a constraints.TokenAutomaton),
logit_bias= / set_logit_bias() and set_token_mask() put layer_ops.constrain_logits behind it and
layer_ops.constraint_advance behind the pick: each stream's automaton state lives on the device and
follows the emitted tokens, drafts included.  One GPU only; no beams.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Union

import torch

from . import layer_ops as _ops

STOP_CHECK_EVERY = 16   # generate(): steps between host looks at the history


def prepare_for_decode(model, *, fuse: bool = True, layer_ops: bool = True, prenorm: bool = True, glue: bool = True,
                       lm_head: bool = True) -> dict:
    """The single-GPU decode layout of a model after replace_with_bnb_linear, in the benchmark's
    order: one grouped GEMV per q/k/v and gate/up set, the one-launch layer ops (norms, rotary,
    attention, residual adds, the MLP pair), the RMSNorms absorbed into the grouped launches, the
    step's mask and rotary tables, and the dense lm_head GEMV.  Returns the number of patches of
    each kind.  A second call patches nothing and returns the first call's counts."""
    done = model.__dict__.get("_qz_prepared")
    if done is not None:
        return dict(done)
    from . import integration as I

    counts = {"groups": 0, "layer_ops": 0, "prenorm": 0, "glue": 0, "lm_head": 0}
    if fuse:
        counts["groups"] = I.fuse_projection_groups(model)
    if layer_ops:
        counts["layer_ops"] = I.fuse_layer_ops(model)
        if prenorm and fuse:
            counts["prenorm"] = I.fuse_prenorm(model)
        if glue:
            counts["glue"] = I.fuse_decode_glue(model)
        if lm_head:
            counts["lm_head"] = I.fuse_lm_head(model)
    model.__dict__["_qz_prepared"] = dict(counts)
    return counts


def _per_stream(value, batch: int, dtype, device, name: str) -> torch.Tensor:
    t = torch.as_tensor(value, dtype=dtype).reshape(-1)
    if t.numel() == 1:
        t = t.expand(batch)
    if t.numel() != batch:
        raise ValueError(f"{name}: one value or one per stream ({batch}), got {t.numel()}")
    return t.to(device)


_PENALTIES = (   # set_penalties()' argument, the session's buffer, its dtype, the neutral value
    ("repetition_penalty", "repetition_penalty", torch.float32, 1),
    ("presence_penalty", "presence_penalty", torch.float32, 0),
    ("frequency_penalty", "frequency_penalty", torch.float32, 0),
    ("no_repeat_ngram_size", "no_repeat_ngram", torch.int32, 0),
    ("min_new_tokens", "min_new_tokens", torch.int64, 0),
)


def _penalty_buffers(sess, batch: int, dev) -> None:
    """The processors' device buffers, neutral, and the host's knowledge of them."""
    sess.repetition_penalty = torch.ones(batch, dtype=torch.float32, device=dev)
    sess.presence_penalty = torch.zeros(batch, dtype=torch.float32, device=dev)
    sess.frequency_penalty = torch.zeros(batch, dtype=torch.float32, device=dev)
    sess.no_repeat_ngram = torch.zeros(batch, dtype=torch.int32, device=dev)
    sess.min_new_tokens = torch.zeros(batch, dtype=torch.int64, device=dev)
    sess.prompt_len = torch.zeros(batch, dtype=torch.int64, device=dev)
    sess._neutral = {name: True for name, _, _, _ in _PENALTIES}
    sess._processing = False   # host knowledge: some processor is on, so the step holds process_logits


PROMPT_LOGPROBS_SLAB = 128   # prompt rows per lm_head + token_logprobs call: 128 x V 16-bit logits (31.3 MiB at V = 128256)


def _check_logprobs(logprobs, who: str) -> Optional[int]:
    if logprobs is None:
        return None
    if isinstance(logprobs, bool) or not isinstance(logprobs, int) or not 0 <= logprobs <= _ops.LOGPROBS_MAX_TOP:
        raise ValueError(f"{who}: logprobs must be None or an integer in 0..{_ops.LOGPROBS_MAX_TOP}, not {logprobs!r}")
    return logprobs


def _logprob_buffers(sess, logprobs, who: str) -> None:
    """The log-probability tables of a session opened with `logprobs`, aligned with sess.hist: NaN / -1
    where there is nothing.  Without it no buffer exists and every hook below returns at once."""
    sess._lp_n = n = _check_logprobs(logprobs, who)
    sess.logprobs = sess.top_ids = sess.top_logprobs = sess._pos0 = None
    if n is None:
        return
    B, L, dev = sess.batch, sess.max_len, sess.device
    sess.logprobs = torch.full((B, L), float("nan"), dtype=torch.float32, device=dev)
    sess.top_ids = torch.full((B, L, n), -1, dtype=torch.int32, device=dev)
    sess.top_logprobs = torch.full((B, L, n), float("nan"), dtype=torch.float32, device=dev)
    sess._pos0 = torch.zeros_like(sess.pos)


def _constraint_buffers(sess, constraint, logit_bias_slots, who: str) -> None:
    """The device state of constrained decoding: the automaton's tables and a state per
    stream when the session was opened with `constraint`, bias lists of `logit_bias_slots` entries per
    stream, and the host mask once set_token_mask() made one.  Without any of them no buffer exists and
    every hook below returns at once."""
    from .constraints import TokenAutomaton

    B, dev = sess.batch, sess.device
    sess.vocab = int(sess.model.config.vocab_size)
    sess.constraint, sess._cn, sess.constraint_state = constraint, None, None
    if constraint is not None:
        if not isinstance(constraint, TokenAutomaton):
            raise ValueError(f"{who}: constraint must be a TokenAutomaton")
        if constraint.V != sess.vocab:
            raise ValueError(f"{who}: the automaton is over {constraint.V} tokens, the model over {sess.vocab}")
        sess._cn = constraint.to(dev)
        sess.constraint_state = torch.full((B,), -1, dtype=torch.int32, device=dev)
        if sess._pos0 is None:
            sess._pos0 = torch.zeros_like(sess.pos)   # the snapshot the log-probabilities take, shared
    nb = int(logit_bias_slots or 0)
    if nb < 0:
        raise ValueError(f"{who}: logit_bias_slots must not be negative")
    sess.logit_bias_slots = nb
    sess._bias_ids = sess._bias_vals = sess._bias_n = sess._token_mask = None
    if nb:
        sess._bias_ids = torch.zeros((B, nb), dtype=torch.int32, device=dev)
        sess._bias_vals = torch.zeros((B, nb), dtype=torch.float32, device=dev)
        sess._bias_n = torch.zeros(B, dtype=torch.int32, device=dev)
    sess._bias_count = [0] * B     # host knowledge of bias_n
    # host knowledge: the step holds constrain_logits (with every operand that exists by then)
    sess._constraining = constraint is not None


def _given_bias(logit_bias, suppress_tokens, batch: int, who: str):
    """generate()'s logit_bias (a dict, or one per stream) and suppress_tokens (ids, -inf for every
    stream) as one dict per stream, or None when neither was given."""
    if logit_bias is None and suppress_tokens is None:
        return None
    if logit_bias is None:
        per = [{} for _ in range(batch)]
    elif hasattr(logit_bias, "items"):
        per = [dict(logit_bias) for _ in range(batch)]
    else:
        per = [dict(d or {}) for d in logit_bias]
        if len(per) != batch:
            raise ValueError(f"{who}: logit_bias is one dict or one per stream ({batch}), got {len(per)}")
    for t in ([] if suppress_tokens is None else suppress_tokens):
        for d in per:
            d[int(t)] = float("-inf")
    return per


def _open_constraints(sess, bias) -> None:
    """generate()'s part after the session is open: the bias lists."""
    if bias is not None:
        for b, d in enumerate(bias):
            sess.set_logit_bias(b, d)


class GenerateOutput(NamedTuple):
    """What generate() / generate_ragged() return when `logprobs` is given: tensors for generate(), one
    tensor per prompt for generate_ragged().  logprobs[.., c] is the log-probability of sequences[.., c]
    under the model's own distribution (NaN on prompt columns), top_ids / top_logprobs[.., c, :] the most
    likely tokens there."""
    sequences: object
    logprobs: object
    top_ids: object
    top_logprobs: object


class DecodeSession:
    """One batch of decode streams over `model`: the StaticCache and the static buffers a captured
    step reads and writes -- tok [B, 1], pos [1], hist [B, max_len] (int64), uniform [B, max_len],
    temperature / top_p [B] (float32), top_k [B] (int32), and the processors' repetition_penalty /
    presence_penalty / frequency_penalty [B] (float32), no_repeat_ngram [B] (int32), min_new_tokens /
    prompt_len / stop [B] (int64; stop is the EOS min_new_tokens holds back, -1: none).  hist holds
    the sequence itself (prompt, then the picked tokens); pos is the position of `tok`, the newest
    token, which the next step feeds: that step writes its pick to hist[:, pos + 1], drawing it with uniform[:, pos], and advances
    pos.  prefill() runs the prompt and picks the first new token.

    logprobs (None: off -- no buffer, launch or graph node; 0: the chosen tokens; 1..20: that many top
    entries too): `logprobs` float32 [B, max_len], `top_ids` int32 and `top_logprobs` float32
    [B, max_len, n], aligned with hist -- entry [b, c] describes token hist[b, c], NaN / -1 where there
    is none (prompt columns, columns not reached).  The model's own distribution: the log-softmax of
    the lm_head row before penalties, temperature, top-k and top-p.  One layer_ops.logprobs_streams
    call follows every pick, inside the captured step; the tokens are those of the session without.

    constraint (a constraints.TokenAutomaton; None: off -- no buffer, launch or graph node) keeps every
    stream's output inside the automaton: `constraint_state` int32 [B] is each stream's state (-1:
    unconstrained, -2: a refused token was taken), prefill(constraint_start=) sets it, one
    layer_ops.constrain_logits call in front of every pick (behind the penalties) turns the logits of the
    tokens the state refuses into -inf, one layer_ops.constraint_advance call behind it moves the state
    over the picked token -- both inside the captured step, no host work per replay.
    logit_bias_slots = NB makes room for NB bias entries per stream (set_logit_bias), set_token_mask()
    takes a host-computed bitmask; both ride in the same launch."""

    def __init__(self, model, batch: int, max_len: int, *, graph: bool = True, logprobs: Optional[int] = None,
                 constraint=None, logit_bias_slots: int = 0):
        from transformers.cache_utils import StaticCache

        if batch < 1 or max_len < 1:
            raise ValueError("DecodeSession: batch and max_len must be positive")
        _check_logprobs(logprobs, "DecodeSession")
        self.model, self.batch, self.max_len = model, int(batch), int(max_len)
        self.device = next(model.parameters()).device
        self.graph = bool(graph) and self.device.type == "cuda"
        dev = self.device
        # two slots of slack: the capture's warm-up runs write the cache at pos and pos + 1
        self.cache = StaticCache(config=model.config, max_cache_len=self.max_len + 2)
        self.tok = torch.zeros((batch, 1), dtype=torch.int64, device=dev)
        self.pos = torch.zeros(1, dtype=torch.int64, device=dev)
        # the pick kernels write hist[b, *pos] and read uniform[b, *pos] (the bench's convention: the
        # column of the token that was fed), so they get the history shifted by one element: column
        # p of `_hist_next` is column p + 1 of the sequence.  Two columns of slack, like the cache.
        width = max_len + 2
        store = torch.zeros(batch * width + 1, dtype=torch.int64, device=dev)
        self._hist_full = store[:batch * width].view(batch, width)
        self._hist_next = store[1:].view(batch, width)
        self.hist = self._hist_full[:, :max_len]
        self._uniform_full = torch.zeros((batch, width), dtype=torch.float32, device=dev)
        self.uniform = self._uniform_full[:, :max_len]
        self.temperature = torch.zeros(batch, dtype=torch.float32, device=dev)   # greedy until set_sampling
        self.top_k = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.top_p = torch.ones(batch, dtype=torch.float32, device=dev)
        self.stop = torch.full((batch,), -1, dtype=torch.int64, device=dev)
        _penalty_buffers(self, batch, dev)
        self._pos_ids = self.pos.view(1, 1).expand(batch, 1)
        self._graph = None
        self._greedy_only = True   # host knowledge: no stream has a temperature > 0
        self._prefilled = False
        self._next = 0   # tokens in hist (host copy of pos + 1)
        _logprob_buffers(self, logprobs, "DecodeSession")
        _constraint_buffers(self, constraint, logit_bias_slots, "DecodeSession")

    def set_sampling(self, temperature=None, top_k=None, top_p=None) -> None:
        """Scalars or one value per stream, written in place: the next step, replayed or not, uses
        them.  temperature <= 0 makes a stream greedy.  A graph captured while every stream was greedy
        holds greedy_step alone, so a stream cannot start sampling after that capture."""
        if temperature is not None:
            t = _per_stream(temperature, self.batch, torch.float32, self.device, "temperature")
            sampled = bool((t > 0).any())
            if self._graph is not None and self._greedy_only and sampled:
                raise ValueError("set_sampling: this session captured a greedy-only step")
            self.temperature.copy_(t)
            if self._graph is None:
                self._greedy_only = not sampled
        if top_k is not None:
            self.top_k.copy_(_per_stream(top_k, self.batch, torch.int32, self.device, "top_k"))
        if top_p is not None:
            self.top_p.copy_(_per_stream(top_p, self.batch, torch.float32, self.device, "top_p"))

    def set_penalties(self, repetition_penalty=None, presence_penalty=None, frequency_penalty=None,
                      no_repeat_ngram_size=None, min_new_tokens=None) -> None:
        """Scalars or one value per stream, written in place like set_sampling: repetition_penalty > 0
        (transformers' rule over every token of the history; 1: off), presence_penalty /
        frequency_penalty (vLLM's rule over the generated tokens; 0: off), no_repeat_ngram_size >= 0 (0:
        off), min_new_tokens >= 0 (holds the stream's `stop` token back; 0: off).  The next step, replayed
        or not, uses them.  A graph captured while every value was neutral holds no processing launch, so
        a processor cannot be switched on after that capture; one captured with any processor on follows
        every later change, back to neutral included."""
        given = dict(repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                     frequency_penalty=frequency_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                     min_new_tokens=min_new_tokens)
        new = {}
        for name, buf, dt, neutral in _PENALTIES:
            if given[name] is None:
                continue
            t = _per_stream(given[name], self.batch, dt, "cpu", name)
            if dt == torch.float32 and not bool(torch.isfinite(t).all()):
                raise ValueError(f"set_penalties: {name} must be finite")
            if name == "repetition_penalty" and not bool((t > 0).all()):
                raise ValueError("set_penalties: repetition_penalty must be positive")
            if name in ("no_repeat_ngram_size", "min_new_tokens") and bool((t < 0).any()):
                raise ValueError(f"set_penalties: {name} must not be negative")
            new[name] = (buf, t, bool((t == neutral).all()))
        if self._graph is not None and not self._processing and not all(n for _, _, n in new.values()):
            raise ValueError("set_penalties: this session captured a step without logits processing")
        for name, (buf, t, neutral) in new.items():
            getattr(self, buf).copy_(t)
            self._neutral[name] = neutral
        if self._graph is None:
            self._processing = not all(self._neutral.values())

    def _process(self, logits: torch.Tensor, rows: slice = slice(None), tok: Optional[torch.Tensor] = None) -> None:
        """layer_ops.process_logits in front of a pick, when some processor is on: in place on the
        rows the pick reads (logits [B, V], or [B*T, V] with the window's tok [B, T])."""
        if not self._processing:
            return
        r = rows
        _ops.process_logits(logits, self._hist_full[r], self.pos if self.pos.numel() == 1 else self.pos[r], tok,
                            repetition_penalty=self.repetition_penalty[r], presence_penalty=self.presence_penalty[r],
                            frequency_penalty=self.frequency_penalty[r], no_repeat_ngram=self.no_repeat_ngram[r],
                            min_new_tokens=self.min_new_tokens[r], prompt_len=self.prompt_len[r], eos=self.stop[r])

    def seed(self, generator: Union[torch.Generator, int, None]) -> None:
        """Refill `uniform` (one number in [0, 1) per stream and position) with torch.rand; the token
        at sequence index i is drawn with uniform[:, i - 1]."""
        if isinstance(generator, int):
            generator = torch.Generator(device=self.device).manual_seed(generator)
        if generator is None:
            self.uniform.copy_(torch.rand(self.uniform.shape, device=self.device))
        else:
            self.uniform.copy_(torch.rand(self.uniform.shape, generator=generator, device=generator.device))

    def _raw_rows(self, logits: torch.Tensor) -> Optional[torch.Tensor]:
        """In front of a pick, in a session with `logprobs`: snapshot pos and return the rows the
        log-probabilities are read from -- the logits themselves, or a copy of them when a processing
        launch is about to rewrite them in place (B T V 16-bit elements, one captured copy)."""
        if self._pos0 is None:
            return None
        self._pos0.copy_(self.pos)       # shared with constraint_advance: a constrained session has one too
        if self._lp_n is None:
            return None
        return logits.clone() if (self._processing or self._constraining) else logits

    def _record(self, raw: Optional[torch.Tensor], rows: slice = slice(None), T: int = 1) -> None:
        """Behind a pick: the log-probabilities of the tokens it emitted (columns pos0 + 1 .. pos of
        hist), from the model's own rows."""
        if raw is None:
            return
        r, n = rows, self._lp_n
        _ops.logprobs_streams(raw, self.hist[r], self._pos0[r], self.pos[r], self.logprobs[r],
                              self.top_ids[r] if n else None, self.top_logprobs[r] if n else None, T)

    def _lp_state(self) -> list:
        """The tables and the snapshot: a capture's warm-up runs write them, _capture() puts them back."""
        return [] if self._lp_n is None else [self.logprobs, self.top_ids, self.top_logprobs, self._pos0]

    def _lp_reset(self, b: int) -> None:
        if self._lp_n is not None:
            self.logprobs[b] = float("nan")
            self.top_ids[b] = -1
            self.top_logprobs[b] = float("nan")

    def set_logit_bias(self, b, bias) -> None:
        """Stream b's logit bias ({token id: bias}; b None: every stream), copied in place into the
        session's bias lists (logit_bias_slots entries per stream), so the next step, replayed or not,
        uses it.  A bias is finite or -inf (a ban); an empty dict clears the list.  The bias is added to
        the stream's logits in front of every pick, behind the penalties; `logprobs` stay the model's
        own.  A step captured with no constraint, bias or mask holds no launch for it: a bias cannot be
        switched on after that capture."""
        from .constraints import bias_row

        ids, vals = bias_row(bias, self.vocab)
        rows = range(self.batch) if b is None else [int(b)]
        if any(not 0 <= r < self.batch for r in rows):
            raise ValueError(f"set_logit_bias: stream {b} outside 0..{self.batch - 1}")
        if len(ids) > self.logit_bias_slots:
            raise ValueError(f"set_logit_bias: {len(ids)} entries, the session was opened with logit_bias_slots="
                             f"{self.logit_bias_slots}")
        if ids and self._graph is not None and not self._constraining:
            raise ValueError("set_logit_bias: this session captured a step without constrained decoding")
        if not self.logit_bias_slots:
            return
        n = len(ids)
        for r in rows:
            if n:
                self._bias_ids[r, :n] = torch.tensor(ids, dtype=torch.int32, device=self.device)
                self._bias_vals[r, :n] = torch.tensor(vals, dtype=torch.float32, device=self.device)
            self._bias_n[r] = n
            self._bias_count[r] = n
        if self._graph is None:
            self._constraining = self._cn is not None or self._token_mask is not None or any(self._bias_count)

    def set_token_mask(self, mask) -> None:
        """A host-computed bitmask for the next picks (int32 [B, ceil(V/32)], xgrammar's layout: bit
        v & 31 of word v >> 5 set = token v allowed), copied in place, so a replay follows it; None
        allows everything again.  The first call makes the buffer, which has to happen before the step
        is captured.  A SpeculativeSession refuses it: the mask of a window's row i would depend on
        drafts chosen on the device."""
        if hasattr(self, "T"):
            raise ValueError("set_token_mask: a host mask describes one row per stream; SpeculativeSession verifies a "
                             "window per stream (use a TokenAutomaton)")
        words = (self.vocab + 31) // 32
        if mask is None:
            if self._token_mask is not None:
                self._token_mask.fill_(-1)
            return
        m = torch.as_tensor(mask)
        if m.dtype != torch.int32 or m.shape != (self.batch, words):
            raise ValueError(f"set_token_mask: mask must be int32 [{self.batch}, {words}]")
        if self._token_mask is None:
            if self._graph is not None:
                raise ValueError("set_token_mask: this session captured a step without a host mask")
            self._token_mask = torch.full((self.batch, words), -1, dtype=torch.int32, device=self.device)
            self._constraining = True
        self._token_mask.copy_(m)

    def _constrain(self, logits: torch.Tensor, rows: slice = slice(None), tok: Optional[torch.Tensor] = None,
                   T: int = 1) -> None:
        """layer_ops.constrain_logits in front of a pick and behind _process, when a constraint, a bias or
        a mask is on: in place on the rows the pick reads."""
        if not self._constraining:
            return
        r = rows
        auto = self._cn is not None
        _ops.constrain_logits(logits, state=self.constraint_state[r] if auto else None, tok=tok if auto else None,
                              automaton=self._cn, mask=None if self._token_mask is None else self._token_mask[r],
                              bias_ids=None if self._bias_ids is None else self._bias_ids[r],
                              bias_vals=None if self._bias_ids is None else self._bias_vals[r],
                              bias_n=None if self._bias_ids is None else self._bias_n[r], T=T)

    def _advance(self, rows: slice = slice(None)) -> None:
        """Behind a pick (and _record): the automaton states follow the tokens it emitted, columns
        pos0 + 1 .. pos of hist."""
        if self._cn is None:
            return
        r = rows
        one = self.pos.numel() == 1
        _ops.constraint_advance(self.constraint_state[r], self.hist[r], self._pos0 if one else self._pos0[r],
                                self.pos if one else self.pos[r], self._cn)

    def _cn_state(self) -> list:
        """What the advance writes: a capture's warm-up runs move it, _capture() puts it back."""
        return [] if self._cn is None else [self.constraint_state]

    def _cn_start(self, rows, start, who: str, keep: bool = False) -> None:
        """Write the automaton state of the streams `rows` in front of their first pick: `start` is an
        int or one per stream (-1: unconstrained); None is the automaton's start state, or with `keep`
        the state the stream has."""
        rows = list(rows)
        if self._cn is None:
            if start is not None:
                raise ValueError(f"{who}: constraint_start needs a session opened with constraint=")
            return
        if start is None:
            if keep:
                return
            start = self.constraint.starts[0] if self.constraint.starts else 0
        vals = [int(v) for v in torch.as_tensor(start).reshape(-1).tolist()]
        if len(vals) == 1:
            vals = vals * len(rows)
        if len(vals) != len(rows) or any(not -1 <= v < self.constraint.S for v in vals):
            raise ValueError(f"{who}: constraint_start is one state or one per stream, each -1 or in "
                             f"0..{self.constraint.S - 1}")
        self.constraint_state[rows] = torch.tensor(vals, dtype=torch.int32, device=self.device)

    def _pick(self, logits: torch.Tensor) -> None:
        raw = self._raw_rows(logits)
        self._process(logits)
        self._constrain(logits)
        if self._greedy_only and logits.is_cuda:
            _ops.greedy_step(logits, self._hist_next, self.pos, self.tok)
        else:
            _ops.sample_step(logits, self._hist_next, self.pos, self.tok, self.temperature, self.top_k, self.top_p,
                             self._uniform_full)
        self._record(raw)
        self._advance()

    @torch.inference_mode()
    def prefill(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, *,
                constraint_start=None) -> None:
        """Run the prompts ([B, S], equal lengths) and pick each stream's first new token.
        constraint_start (sessions opened with constraint=): the automaton state each stream starts in,
        one for all or one per stream; -1 leaves a stream unconstrained; None is the automaton's start."""
        if attention_mask is not None and not bool(attention_mask.bool().all()):
            raise ValueError("DecodeSession.prefill: padded prompts are not supported (attention_mask holds a zero)")
        if input_ids.dim() != 2 or input_ids.shape[0] != self.batch:
            raise ValueError(f"DecodeSession.prefill: input_ids must be [{self.batch}, S]")
        S = input_ids.shape[1]
        if S < 1 or S >= self.max_len:
            raise ValueError("DecodeSession.prefill: the prompt must be shorter than max_len")
        if self._prefilled:
            raise ValueError("DecodeSession.prefill: a session takes one prompt; open another for the next")
        self._cn_start(range(self.batch), constraint_start, "DecodeSession.prefill")
        ids = input_ids.to(self.device)
        self.hist[:, :S] = ids
        self.pos.fill_(S - 1)                          # the last prompt token; the pick makes it S
        self.prompt_len.fill_(S)
        out = self.model(input_ids=ids, past_key_values=self.cache,
                         cache_position=torch.arange(S, device=self.device), use_cache=True)
        self._pick(out.logits[:, -1])
        self._prefilled = True
        self._next = S + 1

    def _step(self) -> None:
        lo = self.model(input_ids=self.tok, past_key_values=self.cache, cache_position=self.pos,
                        position_ids=self._pos_ids, use_cache=True).logits
        self._pick(lo[:, -1])

    def _cache_lengths(self):
        """Each StaticLayer's device-side length (the decode attention advances it in-kernel)."""
        out = [getattr(layer, "cumulative_length", None) for layer in getattr(self.cache, "layers", [])]
        if not out or not all(isinstance(t, torch.Tensor) for t in out):
            raise RuntimeError("DecodeSession: this transformers StaticCache keeps no per-layer device-side "
                               "cumulative_length to restore after the capture's warm-up runs")
        return out

    def _capture(self) -> None:
        # two warm-up runs on a side stream, as the benchmark does; they advance the cache lengths,
        # pos, tok and hist, which are put back so that no position is consumed (the keys and values
        # they wrote lie past the restored length: masked now, overwritten by the steps that follow)
        state = [self.tok, self.pos, self._hist_full] + self._cache_lengths() + self._lp_state() + self._cn_state()
        saved = [t.clone() for t in state]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._step()
        torch.cuda.current_stream().wait_stream(s)
        for t, v in zip(state, saved):
            t.copy_(v)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step()
        for t, v in zip(state, saved):
            t.copy_(v)
        self._graph = g

    @torch.inference_mode()
    def step(self) -> None:
        """One token per stream: the forward of `tok` at position `pos`, the pick,
        hist[:, pos + 1] = tok = token, pos += 1.  With graph=True the first call captures the step and every call replays it."""
        if not self._prefilled:
            raise ValueError("DecodeSession.step: prefill first")
        if self._next >= self.max_len:
            raise ValueError("DecodeSession.step: the history is full (max_len tokens)")
        self._next += 1
        if not self.graph:
            self._step()
            return
        if self._graph is None:
            self._capture()
        self._graph.replay()


@torch.inference_mode()
def generate(model, input_ids: torch.Tensor, max_new_tokens: int, *, do_sample: bool = False,
             temperature: Union[float, Sequence[float]] = 1.0, top_k: Union[int, Sequence[int]] = 0,
             top_p: Union[float, Sequence[float]] = 1.0, generator=None, eos_token_id: Optional[int] = None,
             attention_mask: Optional[torch.Tensor] = None, graph: bool = True,
             prompt_lookup_num_tokens: Optional[int] = None,
             max_matching_ngram_size: Optional[int] = None, prompt_lookup_sampling: bool = False,
             repetition_penalty=None, presence_penalty=None, frequency_penalty=None,
             no_repeat_ngram_size=None, min_new_tokens=None, logprobs: Optional[int] = None,
             constraint=None, constraint_start=None, logit_bias=None, suppress_tokens=None):
    """input_ids [B, S] (equal-length prompts) followed by up to max_new_tokens picked tokens per
    stream: greedy, or with do_sample temperature / top_k / top_p (scalars or one per stream; a
    temperature <= 0 keeps that stream greedy) drawn from `generator` (a torch.Generator or a seed).
    With eos_token_id the history is looked at on the host every 16 steps: a stream's tokens after
    its first EOS are that EOS, and the call returns once every stream has stopped.  Returns int64
    [B, S + new] on the model's device.
    prompt_lookup_num_tokens (transformers' name): verify that many prompt-lookup drafts per stream
    and step in a SpeculativeSession (suffixes of up to max_matching_ngram_size tokens, default 2).
    Greedy unless prompt_lookup_sampling=True, which with do_sample accepts a draft when it is the token
    the row's uniform number draws (SpeculativeSession(sample=True): the tokens of the one-token sampler
    over the same numbers, whatever the drafts).  It needs prepare_for_decode()'s layout on one GPU; the
    result has the shape and the EOS fill the plain call defines.
    repetition_penalty, presence_penalty, frequency_penalty, no_repeat_ngram_size, min_new_tokens
    (scalars or one per stream; None: off): set_penalties() -- the processors run inside the step, in
    front of the pick, with or without prompt lookup; min_new_tokens holds eos_token_id back and does
    nothing without one.
    logprobs (None: off; 0: the chosen tokens only; 1..20: that many top entries as well): return a
    GenerateOutput(sequences, logprobs [B, S + new], top_ids / top_logprobs [B, S + new, n]) aligned
    with the sequences -- the model's own log-softmax, before penalties, temperature, top-k and top-p;
    NaN / -1 on the prompt columns and behind a stream's EOS.
    constraint (a TokenAutomaton) with constraint_start (a state, or one per stream; -1: that stream is
    unconstrained; None: the automaton's start): every pick is masked by its stream's state inside the
    step, with or without prompt lookup.  logit_bias ({token id: bias}, or one dict per stream; -inf
    bans) and suppress_tokens (ids banned for every stream) are added in front of every pick."""
    if input_ids.dim() != 2:
        raise ValueError("generate: input_ids must be [B, S]")
    _check_logprobs(logprobs, "generate")
    B, S = input_ids.shape
    if prompt_lookup_num_tokens is None and max_matching_ngram_size is not None:
        raise ValueError("generate: max_matching_ngram_size needs prompt_lookup_num_tokens")
    if prompt_lookup_num_tokens is not None and do_sample and not prompt_lookup_sampling:
        raise ValueError("generate: prompt_lookup_num_tokens verifies drafts against the greedy token; "
                         "do_sample is not supported with it unless prompt_lookup_sampling=True")
    if max_new_tokens < 1:
        if logprobs is None:
            return input_ids.clone()
        dev = input_ids.device
        return GenerateOutput(input_ids.clone(), torch.full((B, S), float("nan"), device=dev),
                              torch.full((B, S, logprobs), -1, dtype=torch.int32, device=dev),
                              torch.full((B, S, logprobs), float("nan"), device=dev))
    penalties = _given_penalties(repetition_penalty, presence_penalty, frequency_penalty, no_repeat_ngram_size,
                                 min_new_tokens)
    bias = _given_bias(logit_bias, suppress_tokens, B, "generate")
    if constraint is None and constraint_start is not None:
        raise ValueError("generate: constraint_start needs constraint")
    slots = max((len(d) for d in bias), default=0) if bias is not None else 0
    if prompt_lookup_num_tokens is not None:
        sampling = dict(temperature=temperature, top_k=top_k, top_p=top_p, generator=generator) if do_sample else None
        return _generate_speculative(model, input_ids, max_new_tokens, eos_token_id, attention_mask, graph,
                                     prompt_lookup_num_tokens, max_matching_ngram_size, sampling, penalties, logprobs,
                                     constraint, constraint_start, bias)
    sess = DecodeSession(model, B, S + max_new_tokens, graph=graph, logprobs=logprobs, constraint=constraint,
                         logit_bias_slots=slots)
    _open_constraints(sess, bias)
    if penalties:
        sess.set_penalties(**penalties)
        if eos_token_id is not None:
            sess.stop.fill_(int(eos_token_id))
    if do_sample:
        sess.set_sampling(temperature=temperature, top_k=top_k, top_p=top_p)
        sess.seed(generator)
    sess.prefill(input_ids, attention_mask, constraint_start=constraint_start)        # writes hist[:, S]
    n = 1
    while n < max_new_tokens:
        sess.step()
        n += 1
        if eos_token_id is not None and (n % STOP_CHECK_EVERY == 0):
            new = sess.hist[:, S:S + n].cpu()       # one copy
            if bool((new == eos_token_id).any(1).all()):
                break
    out = sess.hist[:, :S + n].clone()
    tabs = None if logprobs is None else [t[:, :S + n].clone() for t in sess._lp_state()[:3]]
    if eos_token_id is not None:
        new = out[:, S:]
        ended = (new == eos_token_id).cumsum(1) > 0
        if tabs is not None:      # behind a stream's first EOS nothing was emitted
            behind = torch.cat((torch.zeros_like(ended[:, :1]), ended[:, :-1]), 1)
            tabs[0][:, S:][behind] = float("nan")
            tabs[1][:, S:][behind] = -1
            tabs[2][:, S:][behind] = float("nan")
        new[ended] = eos_token_id
    return out if tabs is None else GenerateOutput(out, *tabs)


def _given_penalties(repetition_penalty, presence_penalty, frequency_penalty, no_repeat_ngram_size,
                     min_new_tokens) -> dict:
    """The processor arguments a caller passed, as set_penalties() takes them (empty: none)."""
    given = dict(repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                 frequency_penalty=frequency_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                 min_new_tokens=min_new_tokens)
    return {k: v for k, v in given.items() if v is not None}


def _single_gpu_prepared(model, who: str) -> torch.device:
    """The model's device if it is one GPU and prepare_for_decode() laid the model out; raises otherwise."""
    devices = {p.device for p in model.parameters()} | {b.device for b in model.buffers()}
    if len(devices) != 1:
        raise ValueError(f"{who}: the model must live on one device (found {len(devices)}); multi-GPU layouts "
                         "are not supported")
    dev = next(iter(devices))
    if dev.type != "cuda":
        raise ValueError(f"{who}: per-stream positions run in the HIP decode kernels; the model is on {dev}")
    if not model.__dict__.get("_qz_prepared", {}).get("layer_ops"):
        raise ValueError(f"{who}: call prepare_for_decode(model) first (the fused attention carries the positions)")
    return dev


def _check_kv_dtype(kv_dtype, who: str, kv_pages=0) -> None:
    if kv_dtype is None:
        return
    if kv_dtype != "fp8":
        raise ValueError(f"{who}: kv_dtype must be None (the model's 16-bit dtype) or 'fp8', not {kv_dtype!r}")
    if kv_pages is None:
        raise ValueError(f"{who}: kv_dtype='fp8' is a format of the paged cache's pages; open the session with "
                         "kv_pages (the contiguous StaticCache stays 16-bit)")


class PagedLayer:
    """One layer of a PagedKVCache: the K and V page pools [P, Hkv, 128, D] (kv_dtype="fp8": uint8
    [P, Hkv, 128 (D + 1)]) as keys / values."""

    def __init__(self, keys: torch.Tensor, values: torch.Tensor):
        self.keys, self.values = keys, values


class PagedKVCache:
    """What a paged session hands the decoder as past_key_values: per layer one K and one V pool of
    num_pages pages (zero-filled: a page nobody wrote yet holds finite data).  With position_ids and
    a 4-D mask given, the decoder's forward asks nothing of it, and the fused attention reads
    .layers[i] only; anything that tried to use it as a transformers cache ends in update().
    kv_dtype="fp8": the pools are kv8 byte pools, uint8 [P, Hkv, 128 (D + 1)] -- per (page, kv head) 128 D
    E4M3 codes, then 128 power-of-two scale bytes (csrc/paged_attn.hip) -- which the *_paged_kv8
    launches read and write; a zero-filled page reads as zeros there too.  A page is still pool[page]."""

    def __init__(self, config, num_pages: int, dtype, device, kv_dtype: Optional[str] = None):
        _check_kv_dtype(kv_dtype, "PagedKVCache")
        head_dim = getattr(config, "head_dim", None) or config.hidden_size // config.num_attention_heads
        self.kv_dtype = kv_dtype
        if kv_dtype == "fp8":
            if head_dim not in (64, 128):
                raise ValueError(f"PagedKVCache: kv_dtype='fp8' takes head_dim 64 or 128, not {head_dim}")
            shape = (int(num_pages), config.num_key_value_heads, _ops.KV_PAGE * (head_dim + _ops.KV8_ROW_EXTRA))
            dtype = torch.uint8
        else:
            shape = (int(num_pages), config.num_key_value_heads, _ops.KV_PAGE, head_dim)
        self.layers = [PagedLayer(torch.zeros(shape, dtype=dtype, device=device),
                                  torch.zeros(shape, dtype=dtype, device=device))
                       for _ in range(config.num_hidden_layers)]
        keys = self.layers[0].keys
        self.bytes_per_page = 2 * len(self.layers) * (keys.numel() // shape[0]) * keys.element_size()

    def update(self, *args, **kwargs):
        raise RuntimeError("PagedKVCache: keys and values are written by the paged attention launches "
                           "(_qz_paged); this forward took another path")


def _has_adapter_bank(model) -> bool:
    return any(m.__dict__.get("_qz_adapter_bank") is not None for m in model.modules())


class StreamSession:
    """`batch` decode streams over `model`, each at its own position: the StaticCache
    ([B, Hkv, max_len, D] per layer) and the static buffers a captured step reads and writes -- tok
    [B, 1], pos [B], stop [B], limit [B] (int64), live [B] (int32), hist [B, max_len] (int64),
    uniform [B, max_len], temperature / top_p [B] (float32), top_k [B] (int32), and DecodeSession's
    processor buffers (set_penalties; min_new_tokens holds stop[b] back).

    hist[b] is stream b's sequence; pos[b] is the index of tok[b], its newest token, which the next
    step feeds: that step writes k/v to cache slot pos[b], attends to slots 0..pos[b], writes its pick
    to hist[b, pos[b] + 1] (drawn with uniform[b, pos[b]]) and advances pos[b].  A stream leaves
    (live[b] = 0) after writing its stop token or once pos[b] reaches limit[b]; from then on the
    step writes nothing of it, and admit() may hand its row to another prompt.  The graph is
    captured once: positions, liveness, stop tokens, limits and sampling parameters are all read on
    the device.

    prefill_chunk (None: everything as it was): an int c >= 1 runs prompts through
    layer_ops.prefill_attention in windows of c tokens, one model forward per window -- attention
    over the visible keys only, no [T, max_len] mask, activations sized by c, the lm_head on one row
    per stream -- lets admit() write straight into row b of the session's cache, and opens extend().

    kv_pages (None: everything as it was): an int N keeps the keys and values in N pages of 128
    positions per layer (PagedKVCache) in place of the StaticCache, named by one page table
    (kv_pages.KVPagePool, `self.pages`) that the three paged attention launches read on the device.
    It needs prefill_chunk: the paged prompt path is the prefill attention.  prefill(), admit(),
    extend() and fork() reserve a stream's pages up to its limit (plus the draft window of a
    SpeculativeSession) before they run anything, and raise kv_pages.KVPagesExhausted with the session
    unchanged when the pool cannot supply them, so a captured step never needs a page it does not
    have.  release(b) retires a stream and returns its pages; fork(src, dst) continues one stream in
    a second row for the cost of one page copy per layer.  prefix_cache=True publishes each prompt's
    full pages and lets admit() map the resident pages of an equal prefix into the new row, running
    the windows behind them only.  None of this recaptures: the table is a device buffer.
    A shared page carries the bits its donor computed; a newcomer's tokens equal those of its own
    full prefill bit for bit when the donor ran the same windows.

    kv_dtype (None: the model's 16-bit dtype; "fp8" needs kv_pages): the pages hold kv8 rows, D E4M3
    codes and one power-of-two scale byte per row, in (D + 1) / 2D of the bytes; everything above works
    unchanged, and a step scores the new token as every later step reads it back.

    logprobs: DecodeSession's tables, per stream: a stream that is not live has nothing written, admit(b)
    resets row b's columns to NaN / -1, fork(src, dst) copies them, extend() keeps them.
    prompt_logprobs=True (needs prefill_chunk and logprobs): the windows of prefill() / admit() / extend()
    fill the prompt columns 1..S-1 too, the lm_head and layer_ops.token_logprobs over
    PROMPT_LOGPROBS_SLAB window rows at a time (the logits scratch is that many rows x V, never B S x V).
    Column 0 stays NaN, and so do the columns of pages mapped from the prefix cache (no forward ran
    there) and the first column behind them.

    constraint / logit_bias_slots: DecodeSession's, per stream: prefill(), admit() and extend() take
    constraint_start (admit under a captured graph follows it without recapture; extend's None keeps the
    state, and the appended tokens do not advance it), fork(src, dst) copies the state, and a stream
    that is not live keeps its state."""

    def __init__(self, model, batch: int, max_len: int, *, graph: bool = True, prefill_chunk: Optional[int] = None,
                 kv_pages: Optional[int] = None, prefix_cache: bool = False, kv_dtype: Optional[str] = None,
                 logprobs: Optional[int] = None, prompt_logprobs: bool = False, constraint=None,
                 logit_bias_slots: int = 0):
        _check_kv_dtype(kv_dtype, "StreamSession", kv_pages)
        _check_logprobs(logprobs, "StreamSession")
        if prompt_logprobs and prefill_chunk is None:
            raise ValueError("StreamSession: prompt_logprobs needs prefill_chunk (the prompt's rows are scored "
                             "window by window)")
        if prompt_logprobs and logprobs is None:
            raise ValueError("StreamSession: prompt_logprobs fills the tables `logprobs` opens; give logprobs too")
        if batch < 1 or max_len < 2:
            raise ValueError("StreamSession: batch must be positive and max_len at least 2")
        if prefill_chunk is not None and int(prefill_chunk) < 1:
            raise ValueError("StreamSession: prefill_chunk must be None or at least 1")
        if kv_pages is not None and prefill_chunk is None:
            raise ValueError("StreamSession: kv_pages needs prefill_chunk (the paged prompt path is the prefill "
                             "attention)")
        if prefix_cache and kv_pages is None:
            raise ValueError("StreamSession: prefix_cache shares pages; open the session with kv_pages")
        self.prefill_chunk = None if prefill_chunk is None else int(prefill_chunk)
        self.device = _single_gpu_prepared(model, "StreamSession")
        from transformers.cache_utils import StaticCache

        self.model, self.batch, self.max_len = model, int(batch), int(max_len)
        self.graph = bool(graph)
        dev = self.device
        self.pages, self.prefix_cache, self._extra = None, bool(prefix_cache), {}
        if kv_pages is not None:
            from .kv_pages import KVPagePool

            self.pages = KVPagePool(int(kv_pages), self.batch, -(-self.max_len // _ops.KV_PAGE), dev)
            self.cache = PagedKVCache(model.config, int(kv_pages), model.get_input_embeddings().weight.dtype, dev,
                                      kv_dtype=kv_dtype)
            self._extra = {"_qz_paged": (self.pages.table,)}
        else:
            self.cache = StaticCache(config=model.config, max_cache_len=self.max_len)
        self._scratch = None   # admit()'s batch-1 StaticCache, made on first use
        self.tok = torch.zeros((batch, 1), dtype=torch.int64, device=dev)
        self.pos = torch.zeros(batch, dtype=torch.int64, device=dev)
        self.live = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.stop = torch.full((batch,), -1, dtype=torch.int64, device=dev)
        self.limit = torch.zeros(batch, dtype=torch.int64, device=dev)
        # DecodeSession's shift by one: the picks write hist[b, pos[b]], the sequence wants
        # pos[b] + 1.  One column of slack: a live stream has pos[b] + 1 <= limit[b] <= max_len - 1.
        width = max_len + 1
        store = torch.zeros(batch * width + 1, dtype=torch.int64, device=dev)
        self._hist_full = store[:batch * width].view(batch, width)
        self._hist_next = store[1:].view(batch, width)
        self.hist = self._hist_full[:, :max_len]
        self._uniform_full = torch.zeros((batch, width), dtype=torch.float32, device=dev)
        self.uniform = self._uniform_full[:, :max_len]
        self.temperature = torch.zeros(batch, dtype=torch.float32, device=dev)   # greedy until set_sampling
        self.top_k = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.top_p = torch.ones(batch, dtype=torch.float32, device=dev)
        _penalty_buffers(self, batch, dev)
        self._pos_ids = self.pos.view(batch, 1)
        # a constant 4-D bool mask: create_causal_mask hands a 4-D mask back as it is (no launch),
        # and decode_attention_streams takes none -- visibility is j <= pos[b]
        self._mask = torch.ones((batch, 1, 1, self.max_len), dtype=torch.bool, device=dev)
        self._graph = None
        self._greedy_only = True
        self._prefilled = False
        self.prompt_logprobs = bool(prompt_logprobs)
        _logprob_buffers(self, logprobs, "StreamSession")
        _constraint_buffers(self, constraint, logit_bias_slots, "StreamSession")

    set_sampling = DecodeSession.set_sampling
    set_penalties = DecodeSession.set_penalties
    _process = DecodeSession._process
    seed = DecodeSession.seed
    _raw_rows = DecodeSession._raw_rows
    _record = DecodeSession._record
    _lp_state = DecodeSession._lp_state
    _lp_reset = DecodeSession._lp_reset
    set_logit_bias = DecodeSession.set_logit_bias
    set_token_mask = DecodeSession.set_token_mask
    _constrain = DecodeSession._constrain
    _advance = DecodeSession._advance
    _cn_state = DecodeSession._cn_state
    _cn_start = DecodeSession._cn_start

    def _pick(self, logits: torch.Tensor, rows: slice = slice(None)) -> None:
        r = rows
        raw = self._raw_rows(logits)
        self._process(logits, r)
        self._constrain(logits, r)
        if self._greedy_only:
            _ops.greedy_step_streams(logits, self._hist_next[r], self.pos[r], self.live[r], self.stop[r],
                                     self.limit[r], self.tok[r])
        else:
            _ops.sample_step_streams(logits, self._hist_next[r], self.pos[r], self.live[r], self.stop[r],
                                     self.limit[r], self.tok[r], self.temperature[r], self.top_k[r], self.top_p[r],
                                     self._uniform_full[r])
        self._record(raw, r)
        self._advance(r)

    def _limit_of(self, length: int, max_new_tokens: Optional[int]) -> int:
        room = self.max_len - length
        n = room if max_new_tokens is None else int(max_new_tokens)
        if n < 1 or n > room:
            raise ValueError(f"StreamSession: a prompt of {length} tokens has room for 1..{room} new tokens, "
                             f"asked for {n}")
        return length + n - 1   # the stream leaves once pos reaches it: length + n tokens in hist

    def _init_cache(self) -> None:
        """Chunk mode: lay the StaticCache out before the first window (nothing calls its update())."""
        if self.pages is not None:
            return   # the pools are there
        cfg = self.model.config
        head_dim = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
        dtype = self.model.get_input_embeddings().weight.dtype
        self.cache.early_initialization(self.batch, cfg.num_key_value_heads, head_dim, dtype, self.device)

    def _windows(self, ids: torch.Tensor, counts, row0: int, start: int) -> torch.Tensor:
        """Chunk mode: run ids [nb, S] (stream r's first counts[r] columns are real) at positions
        start, start + 1, ... of cache rows row0 .. row0 + nb - 1, in windows of prefill_chunk columns,
        one decoder forward each (windows past the longest count are not run).  Returns the decoder's
        last hidden state at each stream's last real token, [nb, H]."""
        c, dev = self.prefill_chunk, self.device
        nb = ids.shape[0]
        n = torch.as_tensor(counts, dtype=torch.int64, device=dev).reshape(nb)
        top = int(max(counts))
        decoder = self.model.get_decoder()
        one = torch.ones(1, dtype=torch.bool, device=dev)
        rows = torch.arange(nb, device=dev)
        last = None
        for s0 in range(0, top, c):
            T = min(c, top - s0)
            pos = torch.full((nb,), start + s0, dtype=torch.int64, device=dev)
            length = (n - s0).clamp(0, T)
            pids = (start + s0 + torch.arange(T, device=dev)).unsqueeze(0).expand(nb, T).contiguous()
            # create_causal_mask hands a 4-D mask back as it is: an expanded view of one element
            h = decoder(input_ids=ids[:, s0:s0 + T], past_key_values=self.cache, position_ids=pids,
                        attention_mask=one.expand(nb, 1, T, self.max_len), use_cache=True,
                        _qz_prefill=(pos, length, int(row0)), **self._extra).last_hidden_state
            if self.prompt_logprobs:
                self._score_window(h, ids, counts, row0, start, s0, T)
            idx = n - 1 - s0
            mine = h[rows, idx.clamp(0, T - 1)]
            last = mine if last is None else torch.where(((idx >= 0) & (idx < T))[:, None], mine, last)
        return last

    def _score_window(self, h: torch.Tensor, ids: torch.Tensor, counts, row0: int, start: int, s0: int, T: int) -> None:
        """prompt_logprobs: the window's rows (r, j) whose token ids[r, s0 + j] has a prompt token behind
        it score that token -- lm_head and token_logprobs over PROMPT_LOGPROBS_SLAB rows at a time, so
        the logits scratch is slab x V however long the prompts are -- into column start + s0 + j + 1 of
        stream row0 + r's tables.  (The last prompt token's row is the pick's.)"""
        rr, jj = [], []
        for r, cnt in enumerate(counts):
            k = min(T, int(cnt) - 1 - s0)
            if k > 0:
                rr += [r] * k
                jj += range(k)
        if not rr:
            return
        dev, n = self.device, self._lp_n
        rt, jt = torch.tensor(rr, device=dev), torch.tensor(jj, device=dev)
        hid, nxt = h[rt, jt], ids[rt, s0 + jt + 1].contiguous()
        srow, cols = row0 + rt, start + s0 + jt + 1
        head = self.model.get_output_embeddings()
        for a in range(0, len(rr), PROMPT_LOGPROBS_SLAB):
            z = slice(a, a + PROMPT_LOGPROBS_SLAB)
            lp, ti, tl = _ops.token_logprobs(head(hid[z].unsqueeze(0))[0], nxt[z], n)
            self.logprobs[srow[z], cols[z]] = lp
            if n:
                self.top_ids[srow[z], cols[z]] = ti
                self.top_logprobs[srow[z], cols[z]] = tl

    def _slots(self, limit: int) -> int:
        """Cache slots a stream with this limit may write: one per position up to the limit, where a
        retired stream of the captured batch keeps writing, and the draft window of a speculative
        step behind it; rows past the table's end write nothing."""
        return min(limit + getattr(self, "T", 1), self.pages.pages_per_stream * _ops.KV_PAGE)

    def _salt(self, prefix_salt):
        """The registry salt of a call, or False where sharing is off for it: K and V depend on the
        adapter, so a model that carries an adapter bank shares only between calls that name their
        adapter by a salt."""
        if not self.prefix_cache or (prefix_salt is None and _has_adapter_bank(self.model)):
            return False
        return prefix_salt

    def _head(self, hidden: torch.Tensor) -> torch.Tensor:
        """lm_head on one row per stream: [nb, H] -> [nb, V]."""
        return self.model.get_output_embeddings()(hidden.unsqueeze(1))[:, 0]

    @torch.inference_mode()
    def prefill(self, input_ids: torch.Tensor, lengths, *, stop=None, max_new_tokens=None, prefix_salt=None,
                constraint_start=None) -> None:
        """Run right-padded prompts (input_ids [B, Smax], stream b's prompt in its first lengths[b]
        columns) in one forward under the ordinary causal mask -- a real token never sees the pad to
        its right -- and pick each stream's first new token from the logits at lengths[b] - 1.  The
        pad keys left in cache slots lengths[b] .. Smax - 1 lie above pos[b]: invisible, then
        overwritten as the stream grows.  stop: a token id per stream or one for all (None / -1:
        none); max_new_tokens likewise (None: up to max_len).  kv_pages: every stream's pages are
        reserved first (KVPagesExhausted: nothing was changed), and with prefix_cache each prompt's
        full pages are published afterwards under prefix_salt.
        constraint_start (sessions opened with constraint=): the automaton state each stream starts in,
        one for all or one per stream; -1 leaves a stream unconstrained; None is the automaton's start."""
        if self._prefilled:
            raise ValueError("StreamSession.prefill: a session is prefilled once; admit() replaces single streams")
        if input_ids.dim() != 2 or input_ids.shape[0] != self.batch:
            raise ValueError(f"StreamSession.prefill: input_ids must be [{self.batch}, Smax]")
        B, Smax = input_ids.shape
        lens = [int(x) for x in torch.as_tensor(lengths).reshape(-1).tolist()]
        if len(lens) != B or min(lens) < 1 or max(lens) > Smax or Smax > self.max_len:
            raise ValueError("StreamSession.prefill: one length in 1..Smax per stream, Smax <= max_len")
        news = list(max_new_tokens) if isinstance(max_new_tokens, (list, tuple)) else [max_new_tokens] * B
        if len(news) != B:
            raise ValueError("StreamSession.prefill: max_new_tokens is one value or one per stream")
        limits = [self._limit_of(n, m) for n, m in zip(lens, news)]
        dev = self.device
        if self.pages is not None:
            try:
                for b, lim in enumerate(limits):
                    self.pages.reserve(b, self._slots(lim))
            except Exception:
                for b in range(B):
                    self.pages.release(b)
                raise
        self._cn_start(range(B), constraint_start, "StreamSession.prefill")
        ids = input_ids.to(dev)
        ln = torch.tensor(lens, device=dev)
        real = torch.arange(Smax, device=dev)[None, :] < ln[:, None]
        self._hist_full[:, :Smax] = torch.where(real, ids, self._hist_full[:, :Smax])
        self.pos.copy_(ln - 1)
        self.prompt_len.copy_(ln)
        self.limit.copy_(torch.tensor(limits, device=dev))
        self.stop.copy_(_per_stream(-1 if stop is None else stop, B, torch.int64, dev, "stop"))
        self.live.fill_(1)
        if self.prefill_chunk is not None:
            self._init_cache()
            self._pick(self._head(self._windows(ids, lens, 0, 0)))
            self._prefilled = True
            salt = self._salt(prefix_salt)
            if self.pages is not None and salt is not False:
                for b, n in enumerate(lens):
                    self.pages.register(b, ids[b, :n], n // _ops.KV_PAGE, salt, final_below=n)
            return
        out = self.model(input_ids=ids, past_key_values=self.cache,
                         position_ids=torch.arange(Smax, device=dev).unsqueeze(0), use_cache=True)
        self._pick(out.logits[torch.arange(B, device=dev), ln - 1])
        self._prefilled = True

    @torch.inference_mode()
    def admit(self, b: int, prompt: torch.Tensor, *, stop: Optional[int] = None,
              max_new_tokens: Optional[int] = None, prefix_salt=None, constraint_start=None) -> None:
        """Replace stream b by a new prompt (1-D) while the other streams keep their state: the
        prompt runs eagerly at batch 1 into a scratch StaticCache, its keys and values [:S] are copied
        into row b of every layer, and hist[b], pos[b], stop[b], limit[b], live[b] and the stream's
        first token are written.  No recapture: the next replay reads the new state.  With
        prefill_chunk the prompt runs at batch 1 straight against row b of the session's cache, in
        windows: no scratch cache, no copies.
        kv_pages: row b's pages are returned and the new stream's reserved in one step
        (KVPagesExhausted: the session, stream b included, is as it was).  With prefix_cache the
        prompt is looked up first: the resident pages of its longest published prefix -- at most
        (S - 1) // 128, the last prompt token must run -- are mapped into row b and the windows start
        behind them; the prompt's own new full pages are published afterwards.  prefix_salt keeps
        prompts apart whose keys differ for equal tokens (streams on different adapters pass different
        salts); with an adapter bank on the model and no salt, the call shares nothing.
        constraint_start: the new stream's automaton state (-1: unconstrained; None: the automaton's
        start), written like the rest of its state, so the captured step follows it."""
        from transformers.cache_utils import StaticCache

        if not self._prefilled:
            raise ValueError("StreamSession.admit: prefill first (it lays the cache out)")
        if not 0 <= b < self.batch:
            raise ValueError(f"StreamSession.admit: stream {b} outside 0..{self.batch - 1}")
        if prompt.dim() != 1 or prompt.numel() < 1:
            raise ValueError("StreamSession.admit: the prompt must be 1-D and not empty")
        S = prompt.numel()
        limit = self._limit_of(S, max_new_tokens)
        dev = self.device
        ids = prompt.to(dev).view(1, S)
        if self._cn is None and constraint_start is not None:
            raise ValueError("StreamSession.admit: constraint_start needs a session opened with constraint=")
        if self.prefill_chunk is not None:
            start, salt = 0, False
            if self.pages is not None:
                salt = self._salt(prefix_salt)
                hit = self.pages.lookup(ids[0], salt) if salt is not False else []
                self.pages.assign(b, hit, self._slots(limit))
                start = _ops.KV_PAGE * len(hit)
            self._lp_reset(b)
            hidden = self._windows(ids[:, start:], [S - start], b, start)
            self._set_stream(b, ids[0], 0, S, stop, limit)
            self._cn_start([b], constraint_start, "StreamSession.admit")
            self._pick(self._head(hidden), slice(b, b + 1))
            if salt is not False:
                self.pages.register(b, ids[0], S // _ops.KV_PAGE, salt, final_below=S)
            return
        if self._scratch is None:
            self._scratch = StaticCache(config=self.model.config, max_cache_len=self.max_len)
        else:
            self._scratch.reset()
        out = self.model(input_ids=ids, past_key_values=self._scratch,
                         position_ids=torch.arange(S, device=dev).unsqueeze(0), use_cache=True)
        for mine, theirs in zip(self.cache.layers, self._scratch.layers):
            mine.keys[b, :, :S].copy_(theirs.keys[0, :, :S])
            mine.values[b, :, :S].copy_(theirs.values[0, :, :S])
        self._hist_full[b, :S] = ids[0]
        self._lp_reset(b)
        self.pos[b] = S - 1
        self.prompt_len[b] = S
        self.stop[b] = -1 if stop is None else int(stop)
        self.limit[b] = limit
        self.live[b] = 1    # before the pick, which writes live streams only and may retire this one at once
        self._cn_start([b], constraint_start, "StreamSession.admit")
        self._pick(out.logits[:, -1], slice(b, b + 1))

    def _set_stream(self, b: int, tokens: torch.Tensor, at: int, end: int, stop, limit: int) -> None:
        """hist[b, at:end] = tokens; the stream stands at its last token, live, everything so far its prompt."""
        self._hist_full[b, at:end] = tokens
        self.pos[b] = end - 1
        self.prompt_len[b] = end
        self.stop[b] = -1 if stop is None else int(stop)
        self.limit[b] = limit
        self.live[b] = 1    # before the pick, which writes live streams only and may retire this one at once

    @torch.inference_mode()
    def extend(self, b: int, tokens: torch.Tensor, *, stop: Optional[int] = None,
               max_new_tokens: Optional[int] = None, constraint_start=None) -> None:
        """Append tokens (1-D) to stream b's sequence, live or retired -- a conversation's next turn --
        and pick the token after them.  hist[b, pos[b]], the stream's newest token, is not in the cache
        yet: the window is that token followed by `tokens`, at positions pos[b] .., in chunks of
        prefill_chunk against row b of the cache.  Afterwards hist[b] holds the tokens and the stream's
        first new token, picked from the window's last row: pos[b] stands on that token, as after
        admit() -- it has advanced by the number of tokens and then by the pick's own step, n + 1 in
        all -- and stop / limit / live are set as admit() sets them.  The whole sequence so far, the appended
        tokens and the tokens generated before them included, counts as prompt from here on: the
        presence and frequency penalties count what is generated after this call, and min_new_tokens
        starts again.  The other streams keep their state; no recapture.
        constraint_start: None keeps the stream's automaton state (the appended tokens do not advance
        it), a state or -1 replaces it in front of the pick."""
        if self.prefill_chunk is None:
            raise ValueError("StreamSession.extend: open the session with prefill_chunk (the prefill attention "
                             "places the window)")
        if not self._prefilled:
            raise ValueError("StreamSession.extend: prefill first (it lays the cache out)")
        if not 0 <= b < self.batch:
            raise ValueError(f"StreamSession.extend: stream {b} outside 0..{self.batch - 1}")
        if tokens.dim() != 1 or tokens.numel() < 1:
            raise ValueError("StreamSession.extend: the tokens must be 1-D and not empty")
        p, n = int(self.pos[b]), tokens.numel()
        if p + 1 + n >= self.max_len:
            raise ValueError(f"StreamSession.extend: {p + 1} tokens and {n} more leave no room in max_len "
                             f"{self.max_len}")
        limit = self._limit_of(p + 1 + n, max_new_tokens)
        if self.pages is not None:
            self.pages.reserve(b, self._slots(limit))   # KVPagesExhausted: nothing was changed
        new = tokens.to(self.device).view(n)
        ids = torch.cat((self._hist_full[b, p:p + 1], new)).view(1, n + 1)
        hidden = self._windows(ids, [n + 1], b, p)
        self._set_stream(b, new, p + 1, p + 1 + n, stop, limit)
        self._cn_start([b], constraint_start, "StreamSession.extend", keep=True)
        self._pick(self._head(hidden), slice(b, b + 1))

    def _need_pages(self, who: str) -> None:
        if self.pages is None:
            raise ValueError(f"StreamSession.{who}: open the session with kv_pages")
        if not self._prefilled:
            raise ValueError(f"StreamSession.{who}: prefill first")

    @torch.inference_mode()
    def release(self, b: int) -> None:
        """Retire stream b and return its pages (kv_pages sessions).  The row keeps one private page
        and stands at position 0, not live: the captured step goes on computing it on data of its
        own, writes nothing of it to hist, and can never write into a page that was handed on."""
        self._need_pages("release")
        if not 0 <= b < self.batch:
            raise ValueError(f"StreamSession.release: stream {b} outside 0..{self.batch - 1}")
        self.pages.release(b)
        self.live[b] = 0
        self.pos[b] = 0
        if hasattr(self, "_draft"):
            self._draft()   # a speculative session's position ids follow pos

    @torch.inference_mode()
    def fork(self, src: int, dst: int, *, stop: Optional[int] = None, max_new_tokens: Optional[int] = None) -> None:
        """Continue stream src in row dst as well (kv_pages sessions): dst is released, then names
        src's pages below pos[src] >> 7 -- final, since src only writes at its position and above --
        gets a copy of the partial page behind them (every layer, K and V) and src's hist row, tok, pos
        and prompt_len.  It keeps its own sampling parameters, penalties and uniform row: several
        samples of one prompt for one prefill.  stop / max_new_tokens: None takes src's stop token /
        src's limit and liveness.  KVPagesExhausted: the session, row dst included, is as it was."""
        self._need_pages("fork")
        if not (0 <= src < self.batch and 0 <= dst < self.batch) or src == dst:
            raise ValueError(f"StreamSession.fork: two different streams of 0..{self.batch - 1}")
        p = int(self.pos[src])
        limit = int(self.limit[src]) if max_new_tokens is None else self._limit_of(p + 1, max_new_tokens)
        pair = self.pages.fork(src, dst, p, self._slots(limit))
        if pair is not None:
            for layer in self.cache.layers:
                layer.keys[pair[1]].copy_(layer.keys[pair[0]])
                layer.values[pair[1]].copy_(layer.values[pair[0]])
        self._hist_full[dst].copy_(self._hist_full[src])
        for t in self._lp_state()[:3]:
            t[dst].copy_(t[src])
        for t in self._cn_state():
            t[dst].copy_(t[src])
        self.tok[dst].copy_(self.tok[src])
        if hasattr(self, "pos_ids"):
            self.pos_ids[dst].copy_(self.pos_ids[src])
        self.pos[dst] = p
        self.prompt_len[dst] = self.prompt_len[src]
        self.stop[dst] = self.stop[src] if stop is None else int(stop)
        self.limit[dst] = limit
        self.live[dst] = self.live[src] if max_new_tokens is None else 1

    def page_stats(self) -> dict:
        """The pool's pages by state -- free, held (named by a stream), idle (published, named by
        nobody, evictable) and total -- and the bytes one page takes over all layers, K and V."""
        if self.pages is None:
            raise ValueError("StreamSession.page_stats: open the session with kv_pages")
        return dict(self.pages.stats(), bytes_per_page=self.cache.bytes_per_page)

    def _step(self) -> None:
        lo = self.model(input_ids=self.tok, past_key_values=self.cache, position_ids=self._pos_ids,
                        attention_mask=self._mask, use_cache=True, _qz_stream_pos=self.pos, **self._extra).logits
        self._pick(lo[:, -1])

    def _step_state(self) -> list:
        """What a step writes besides the cache: _capture() puts it back after its warm-up runs."""
        return [self.tok, self.pos, self.live, self._hist_full] + self._lp_state() + self._cn_state()

    def _capture(self) -> None:
        # two warm-up runs on a side stream, then the capture; each advances the live streams, which
        # is undone by restoring tok, pos, live and hist (the k/v they wrote at pos + 1 lie above the
        # restored positions: invisible, overwritten by the steps that follow).  No cache length to
        # restore: the streams launch never touches StaticLayer.cumulative_length.
        state = self._step_state()
        saved = [t.clone() for t in state]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._step()
        torch.cuda.current_stream().wait_stream(s)
        for t, v in zip(state, saved):
            t.copy_(v)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step()
        for t, v in zip(state, saved):
            t.copy_(v)
        self._graph = g

    @torch.inference_mode()
    def step(self) -> None:
        """One token for every live stream.  `limit` keeps each stream inside max_len on the device,
        so there is nothing to count here; with graph=True the first call captures the step and every
        call replays it."""
        if not self._prefilled:
            raise ValueError("StreamSession.step: prefill first")
        if not self.graph:
            self._step()
            return
        if self._graph is None:
            self._capture()
        self._graph.replay()

    def alive(self) -> torch.Tensor:
        """Which streams are live: a bool [B] on the host (one device read)."""
        return self.live.cpu() != 0

    def sequences(self) -> list:
        """Each stream's tokens so far, hist[b, :pos[b] + 1], as 1-D int64 tensors (one read of pos)."""
        pos = self.pos.cpu().tolist()
        return [self.hist[b, :p + 1].clone() for b, p in enumerate(pos)]


SPECULATIVE_CHECK_EVERY = 4   # speculative generate: steps between host looks at `live`
PROMPT_LOOKUP_NGRAM = 2       # transformers' default max_matching_ngram_size


class SpeculativeSession(StreamSession):
    """StreamSession that verifies draft_tokens drafts per stream and step, greedy unless sample=True.  tok is
    [B, T] with T = draft_tokens + 1: column 0 is the stream's newest token, columns 1.. are drafts for
    the tokens after it.  A step runs the model on all B T rows in one read of the weights (the window
    is causal within a stream: layer_ops.decode_attention_verify), picks the greedy token of every
    row, and emits row 0's pick and then each further row's pick for as long as the draft that row was
    fed is the token just emitted (layer_ops.verify_step_streams): 1..T tokens per live stream,
    accepted [B] of them.  The tokens are those of StreamSession whatever the drafts were, because
    every launch of the step gives a token the same bits in whichever row it sits.  Rejected rows
    left k/v above the new pos[b]: invisible, overwritten later.  A row past the cache end is NaN and
    is never emitted (pos[b] + i + 1 <= limit[b] <= max_len - 1 for an emitted row i).

    _draft() fills tok[:, 1:] and pos_ids [B, T] = pos[b] + i for the next step; here it is the
    prompt-lookup drafter layer_ops.ngram_draft over the stream's own history with suffixes of up to
    `ngram` tokens.  A subclass may replace it with anything that runs on the device and writes token
    ids of the vocabulary for every stream, live or not (the embedding looks all B T rows up).
    batch * T is at most core.MT_MAX_TOKENS (the multi-token 4-bit kernel's rows).

    sample=True: set_sampling() and seed() as in StreamSession, and a step draws every row with the
    uniform number of the position it sits at (layer_ops.verify_sample_step_streams): row i of stream
    b with uniform[b, pos[b] + i].  A token is a function of its logits row and that number, so the
    emitted tokens are still the same whatever the drafts were, and a stream with temperature <= 0
    stays greedy.  A step captured while every stream was greedy holds the greedy pick alone.

    set_penalties(): the processors run over all B T rows in one launch before the pick, row i with the
    history hist[b, :pos[b] + 1] followed by the drafts 1..i.  An emitted row's drafts are the tokens
    emitted before it, so its history is the real one and the tokens stay StreamSession's.

    constraint: the one constrain_logits launch covers the B T rows, row i masked by the state reached
    from the stream's over the drafts 1..i (walked on the device); a row behind a draft that the row in
    front of it refuses is left alone and is never accepted, and the advance follows the accepted tokens.
    The tokens stay StreamSession's under the same automaton.  set_token_mask() raises here."""

    def __init__(self, model, batch: int, max_len: int, *, draft_tokens: int = 3, ngram: int = 3, graph: bool = True,
                 sample: bool = False, prefill_chunk: Optional[int] = None, kv_pages: Optional[int] = None,
                 prefix_cache: bool = False, kv_dtype: Optional[str] = None, logprobs: Optional[int] = None,
                 prompt_logprobs: bool = False, constraint=None, logit_bias_slots: int = 0):
        from .core import MT_MAX_TOKENS

        if int(draft_tokens) < 1:
            raise ValueError("SpeculativeSession: draft_tokens must be at least 1")
        if not 1 <= int(ngram) <= _ops.NGRAM_MAX:
            raise ValueError(f"SpeculativeSession: ngram must be in 1..{_ops.NGRAM_MAX}")
        T = int(draft_tokens) + 1
        if batch * T > MT_MAX_TOKENS:
            raise ValueError(f"SpeculativeSession: batch * (draft_tokens + 1) = {batch * T} rows per step, the "
                             f"multi-token kernels take {MT_MAX_TOKENS}")
        super().__init__(model, batch, max_len, graph=graph, prefill_chunk=prefill_chunk, kv_pages=kv_pages,
                         prefix_cache=prefix_cache, kv_dtype=kv_dtype, logprobs=logprobs,
                         prompt_logprobs=prompt_logprobs, constraint=constraint, logit_bias_slots=logit_bias_slots)
        dev = self.device
        self.T, self.ngram, self.sample = T, int(ngram), bool(sample)
        self.tok = torch.zeros((batch, T), dtype=torch.int64, device=dev)
        self.pos_ids = torch.zeros((batch, T), dtype=torch.int64, device=dev)
        self.accepted = torch.zeros(batch, dtype=torch.int32, device=dev)
        self._steps = torch.zeros(batch, dtype=torch.int64, device=dev)
        self._tokens = torch.zeros(batch, dtype=torch.int64, device=dev)
        self._mask = torch.ones((batch, 1, T, self.max_len), dtype=torch.bool, device=dev)

    def set_sampling(self, temperature=None, top_k=None, top_p=None) -> None:
        """Without sample=True, greedy only: accepting a draft compares it with THE token of its row.
        With it, StreamSession's set_sampling: the token of a row is the one its uniform number draws."""
        if self.sample:
            return super().set_sampling(temperature=temperature, top_k=top_k, top_p=top_p)
        if temperature is not None and bool((torch.as_tensor(temperature, dtype=torch.float32) > 0).any()):
            raise ValueError("SpeculativeSession: speculative decoding is greedy only (no temperature) unless the "
                             "session was opened with sample=True")

    def _draft(self) -> None:
        _ops.ngram_draft(self._hist_full, self.pos, self.tok, self.pos_ids, self.ngram)

    def _pick(self, logits: torch.Tensor, rows: slice = slice(None)) -> None:
        # prefill() and admit(): one row of logits per stream, the plain pick, then drafts for everyone
        # (a stream whose state did not change gets the drafts it had, or others: they are hints)
        r = rows
        raw = self._raw_rows(logits)
        self._process(logits, r)
        self._constrain(logits, r)
        first = self.tok[r, :1].contiguous()
        if self._greedy_only:
            _ops.greedy_step_streams(logits, self._hist_next[r], self.pos[r], self.live[r], self.stop[r],
                                     self.limit[r], first)
        else:
            _ops.sample_step_streams(logits, self._hist_next[r], self.pos[r], self.live[r], self.stop[r],
                                     self.limit[r], first, self.temperature[r], self.top_k[r], self.top_p[r],
                                     self._uniform_full[r])
        self.tok[r, :1] = first
        self._record(raw, r)
        self._advance(r)
        self._draft()

    def _step(self) -> None:
        lo = self.model(input_ids=self.tok, past_key_values=self.cache, position_ids=self.pos_ids,
                        attention_mask=self._mask, use_cache=True, _qz_verify_pos=self.pos, **self._extra).logits
        lo = lo.reshape(self.batch * self.T, -1)
        raw = self._raw_rows(lo)
        self._process(lo, tok=self.tok)    # row i sees the drafts 1..i it was fed after
        self._constrain(lo, tok=self.tok, T=self.T)   # row i in the state reached over the drafts 1..i
        if self._greedy_only:
            _ops.verify_step_streams(lo, self._hist_next, self.pos, self.live, self.stop, self.limit, self.tok,
                                     self.accepted)
        else:
            _ops.verify_sample_step_streams(lo, self._hist_next, self.pos, self.live, self.stop, self.limit, self.tok,
                                            self.accepted, self.temperature, self.top_k, self.top_p,
                                            self._uniform_full)
        self._record(raw, T=self.T)        # the accepted rows: columns pos0 + 1 .. pos
        self._advance()                    # the states follow the accepted tokens
        self._tokens.add_(self.accepted)
        self._steps.add_(self.accepted.ne(0))
        self._draft()

    def _step_state(self) -> list:
        return super()._step_state() + [self.pos_ids, self.accepted, self._steps, self._tokens]

    def stats(self) -> dict:
        """Running totals per stream, read from the device now: "steps" the steps the stream was live
        in, "tokens" the tokens those steps emitted (prefill's and admit's first tokens are not steps)."""
        return {"steps": self._steps.cpu(), "tokens": self._tokens.cpu()}


def _speculative_session(model, batch: int, max_len: int, prompt_lookup_num_tokens, max_matching_ngram_size,
                         do_sample: bool, graph: bool, who: str, sampling: bool = False,
                         prefill_chunk: Optional[int] = None, kv_pages: Optional[int] = None,
                         kv_dtype: Optional[str] = None, logprobs: Optional[int] = None, constraint=None,
                         logit_bias_slots: int = 0) -> SpeculativeSession:
    if do_sample and not sampling:
        raise ValueError(f"{who}: prompt_lookup_num_tokens verifies drafts against the greedy token; "
                         "do_sample is not supported with it unless prompt_lookup_sampling=True")
    n = PROMPT_LOOKUP_NGRAM if max_matching_ngram_size is None else int(max_matching_ngram_size)
    return SpeculativeSession(model, batch, max_len, draft_tokens=int(prompt_lookup_num_tokens), ngram=n, graph=graph,
                              sample=bool(do_sample and sampling), prefill_chunk=prefill_chunk, kv_pages=kv_pages,
                              kv_dtype=kv_dtype, logprobs=logprobs, constraint=constraint,
                              logit_bias_slots=logit_bias_slots)


def _run_speculative(sess: SpeculativeSession, max_new_tokens: int) -> None:
    """Step until no stream is live: at most max_new_tokens - 1 steps, a host look every few."""
    for n in range(1, max_new_tokens):
        sess.step()
        if n % SPECULATIVE_CHECK_EVERY == 0 and not bool(sess.alive().any()):
            break


def _generate_speculative(model, input_ids, max_new_tokens, eos_token_id, attention_mask, graph,
                          prompt_lookup_num_tokens, max_matching_ngram_size, sampling=None,
                          penalties=None, logprobs=None, constraint=None, constraint_start=None, bias=None):
    """generate()'s result from a SpeculativeSession: every stream runs to its EOS or to max_new_tokens,
    then the rows are laid out as the plain loop leaves them -- S + n columns, n the first multiple of
    STOP_CHECK_EVERY by which every stream had its EOS (max_new_tokens if there is none), each
    stream's tokens after its EOS that EOS.  `sampling` (temperature, top_k, top_p, generator) opens
    the session with sample=True; `penalties` is set_penalties()' arguments."""
    if attention_mask is not None and not bool(attention_mask.bool().all()):
        raise ValueError("generate: padded prompts are not supported (attention_mask holds a zero)")
    B, S = input_ids.shape
    sess = _speculative_session(model, B, S + max_new_tokens, prompt_lookup_num_tokens, max_matching_ngram_size,
                                sampling is not None, graph, "generate", sampling is not None, logprobs=logprobs,
                                constraint=constraint,
                                logit_bias_slots=max((len(d) for d in bias), default=0) if bias is not None else 0)
    _open_constraints(sess, bias)
    if sampling is not None:
        sess.set_sampling(temperature=sampling["temperature"], top_k=sampling["top_k"], top_p=sampling["top_p"])
        sess.seed(sampling["generator"])
    if penalties:
        sess.set_penalties(**penalties)
    sess.prefill(input_ids, [S] * B, stop=eos_token_id, max_new_tokens=max_new_tokens,
                 constraint_start=constraint_start)
    _run_speculative(sess, max_new_tokens)
    seqs = sess.sequences()
    n = max_new_tokens
    if eos_token_id is not None and all(int(s[-1]) == eos_token_id for s in seqs):
        longest = max(s.numel() for s in seqs) - S
        n = min(max_new_tokens, -(-longest // STOP_CHECK_EVERY) * STOP_CHECK_EVERY)
    fill = 0 if eos_token_id is None else eos_token_id
    out = torch.full((B, S + n), fill, dtype=torch.int64, device=sess.device)
    for b, s in enumerate(seqs):
        out[b, :s.numel()] = s
    if logprobs is None:
        return out
    # a stream that stopped wrote nothing more: the tables' columns behind its EOS are still NaN / -1
    return GenerateOutput(out, *(t[:, :S + n].clone() for t in sess._lp_state()[:3]))


@torch.inference_mode()
def generate_ragged(model, prompts: Sequence[torch.Tensor], max_new_tokens: int, *, do_sample: bool = False,
                    temperature: Union[float, Sequence[float]] = 1.0, top_k: Union[int, Sequence[int]] = 0,
                    top_p: Union[float, Sequence[float]] = 1.0, generator=None, eos_token_id: Optional[int] = None,
                    graph: bool = True, prompt_lookup_num_tokens: Optional[int] = None,
                    max_matching_ngram_size: Optional[int] = None, prompt_lookup_sampling: bool = False,
                    repetition_penalty=None, presence_penalty=None, frequency_penalty=None,
                    no_repeat_ngram_size=None, min_new_tokens=None, prefill_chunk: Optional[int] = None,
                    kv_pages: Optional[int] = None, kv_dtype: Optional[str] = None, logprobs: Optional[int] = None,
                    constraint=None, constraint_start=None, logit_bias=None, suppress_tokens=None):
    """generate() for prompts of different lengths: `prompts` are 1-D int64 tensors; returns one 1-D
    int64 tensor per prompt on the model's device, the prompt followed by up to max_new_tokens picked
    tokens of its own, ending with eos_token_id if the stream picked it.  A stream that stopped writes
    nothing more; the host looks at `live` every STOP_CHECK_EVERY steps and returns once none is.
    One GPU and prepare_for_decode()'s layout; anything else raises.
    prompt_lookup_num_tokens (transformers' name): verify that many prompt-lookup drafts per stream
    and step in a SpeculativeSession (suffixes of up to max_matching_ngram_size tokens, default 2) --
    the same tokens in fewer steps wherever the text repeats itself: greedy, or with do_sample and
    prompt_lookup_sampling=True the sampled tokens of SpeculativeSession(sample=True).
    repetition_penalty, presence_penalty, frequency_penalty, no_repeat_ngram_size, min_new_tokens:
    as generate() takes them, one value or one per prompt.
    prefill_chunk: the session's (StreamSession): None keeps the whole-prompt forward, an int runs the
    prompts through layer_ops.prefill_attention in windows of that many tokens.
    kv_pages: the session's: that many pages of 128 positions per layer in place of a cache row of
    Smax + max_new_tokens positions per prompt (needs prefill_chunk).
    kv_dtype: the session's: "fp8" keeps the pages as kv8 rows (needs kv_pages).
    logprobs: as generate() takes it; the GenerateOutput's fields are lists with one tensor per prompt,
    each cut to that prompt's sequence.
    constraint, constraint_start, logit_bias, suppress_tokens: as generate() takes them, one value or one
    per prompt."""
    _check_logprobs(logprobs, "generate_ragged")
    prompts = list(prompts)
    if not prompts or any((not isinstance(p, torch.Tensor)) or p.dim() != 1 or p.numel() < 1 for p in prompts):
        raise ValueError("generate_ragged: prompts must be a non-empty sequence of non-empty 1-D tensors")
    if max_new_tokens < 1:
        raise ValueError("generate_ragged: max_new_tokens must be positive")
    lens = [p.numel() for p in prompts]
    B, Smax = len(prompts), max(lens)
    bias = _given_bias(logit_bias, suppress_tokens, B, "generate_ragged")
    if constraint is None and constraint_start is not None:
        raise ValueError("generate_ragged: constraint_start needs constraint")
    slots = max((len(d) for d in bias), default=0) if bias is not None else 0
    if prompt_lookup_num_tokens is not None:
        sess = _speculative_session(model, B, Smax + max_new_tokens, prompt_lookup_num_tokens,
                                    max_matching_ngram_size, do_sample, graph, "generate_ragged",
                                    prompt_lookup_sampling, prefill_chunk, kv_pages, kv_dtype, logprobs, constraint, slots)
    elif max_matching_ngram_size is not None:
        raise ValueError("generate_ragged: max_matching_ngram_size needs prompt_lookup_num_tokens")
    else:
        sess = StreamSession(model, B, Smax + max_new_tokens, graph=graph, prefill_chunk=prefill_chunk,
                             kv_pages=kv_pages, kv_dtype=kv_dtype, logprobs=logprobs, constraint=constraint,
                             logit_bias_slots=slots)
    _open_constraints(sess, bias)
    if do_sample:
        sess.set_sampling(temperature=temperature, top_k=top_k, top_p=top_p)
        sess.seed(generator)
    penalties = _given_penalties(repetition_penalty, presence_penalty, frequency_penalty, no_repeat_ngram_size,
                                 min_new_tokens)
    if penalties:
        sess.set_penalties(**penalties)
    ids = torch.zeros((B, Smax), dtype=torch.int64, device=sess.device)
    for b, p in enumerate(prompts):
        ids[b, :lens[b]] = p.to(sess.device)
    sess.prefill(ids, lens, stop=eos_token_id, max_new_tokens=max_new_tokens, constraint_start=constraint_start)
    if isinstance(sess, SpeculativeSession):
        _run_speculative(sess, max_new_tokens)
        return _ragged_output(sess)
    n = 1
    while n < max_new_tokens:
        sess.step()
        n += 1
        if eos_token_id is not None and n % STOP_CHECK_EVERY == 0 and not bool(sess.alive().any()):
            break
    return _ragged_output(sess)


def _ragged_output(sess):
    """sequences(), and with `logprobs` the tables' rows cut to them."""
    seqs = sess.sequences()
    if sess._lp_n is None:
        return seqs
    return GenerateOutput(seqs, *([t[b, :s.numel()].clone() for b, s in enumerate(seqs)] for t in sess._lp_state()[:3]))


@torch.inference_mode()
def score(model, prompts: Sequence[torch.Tensor], *, top_logprobs: int = 0, prefill_chunk: int = 512) -> list:
    """Log-probabilities of given texts: `prompts` are 1-D int64 tensors; returns one float32 tensor t
    per prompt on the model's device with t[c] = log p(token_c | tokens_<c) under the model (t[0] is
    NaN: nothing precedes the first token), so (-t[1:].mean()).exp() is the prompt's perplexity.  The
    prompts run through a StreamSession(prefill_chunk=..., prompt_logprobs=True) in windows of
    prefill_chunk tokens, the lm_head over PROMPT_LOGPROBS_SLAB rows at a time; no decode step is
    captured or run.  top_logprobs = n in 1..20: each entry is (t, top_ids [S, n], top_logprobs [S, n])
    instead, the n most likely tokens at every column.  One GPU and prepare_for_decode()'s layout."""
    _single_gpu_prepared(model, "score")
    n = top_logprobs
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= _ops.LOGPROBS_MAX_TOP:
        raise ValueError(f"score: top_logprobs must be an integer in 0..{_ops.LOGPROBS_MAX_TOP}, not {n!r}")
    prompts = list(prompts)
    if not prompts or any((not isinstance(p, torch.Tensor)) or p.dim() != 1 or p.numel() < 1 for p in prompts):
        raise ValueError("score: prompts must be a non-empty sequence of non-empty 1-D tensors")
    if prefill_chunk is None or int(prefill_chunk) < 1:
        raise ValueError("score: prefill_chunk must be at least 1")
    lens = [p.numel() for p in prompts]
    B, Smax = len(prompts), max(lens)
    sess = StreamSession(model, B, Smax + 1, graph=False, prefill_chunk=int(prefill_chunk), logprobs=n,
                         prompt_logprobs=True)
    ids = torch.zeros((B, Smax), dtype=torch.int64, device=sess.device)
    for b, p in enumerate(prompts):
        ids[b, :lens[b]] = p.to(sess.device)
    sess.prefill(ids, lens, max_new_tokens=1)
    if not n:
        return [sess.logprobs[b, :S].clone() for b, S in enumerate(lens)]
    return [(sess.logprobs[b, :S].clone(), sess.top_ids[b, :S].clone(), sess.top_logprobs[b, :S].clone())
            for b, S in enumerate(lens)]
