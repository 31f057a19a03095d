"""CPU: the adapter-bank API of Linear4bit (set_adapter_bank / clear_adapter_bank / adapter_bank,
lora.AdapterBank), the loaders for several peft adapter directories (integration.load_lora_adapters /
replace_lora_adapter / unload_lora_adapter) and the sharding functions' refusal, on a tiny
random-init Llama whose Linear4bit layers were never moved to a GPU (no kernel runs)."""
import copy

import pytest
import torch
from test_lora_host import _model, _write_adapter

QV = ("q_proj", "v_proj")


def _ab(r, out_f=32, in_f=64, seed=0):
    g = torch.Generator().manual_seed(seed + r)
    return torch.randn(r, in_f, generator=g).half(), torch.randn(out_f, r, generator=g).half()


def test_loader_builds_padded_banks_zero_entries_and_shared_slots(tmp_path):
    from quantizations_amd import Linear4bit
    from quantizations_amd.core import MT_MAX_TOKENS
    from quantizations_amd.integration import load_lora_adapters, unload_lora_adapter

    model = _model()
    d0, d1 = str(tmp_path / "a0"), str(tmp_path / "a1")
    t0 = _write_adapter(d0, model, targets=QV, r=4)                       # alpha 8 -> scaling 2
    t1 = _write_adapter(d1, model, targets=("v_proj", "o_proj"), r=8)     # scaling 1
    slots = load_lora_adapters(model, [d0, d1])
    assert slots.dtype == torch.int32 and slots.shape == (MT_MAX_TOKENS,) and bool((slots == -1).all())
    seen = 0
    for name, mod in model.named_modules():
        if not isinstance(mod, Linear4bit):
            continue
        leaf = name.split(".")[-1]
        bank = mod.adapter_bank
        if leaf not in ("q_proj", "v_proj", "o_proj"):
            assert bank is None
            continue
        seen += 1
        assert mod.adapter is None and bank.slots is slots and bank.n == 2
        assert bank.A.is_contiguous() and bank.B.is_contiguous() and bank.scaling.dtype == torch.float32
        a0, b0 = t0.get(f"base_model.model.{name}.lora_A.weight"), t0.get(f"base_model.model.{name}.lora_B.weight")
        a1, b1 = t1.get(f"base_model.model.{name}.lora_A.weight"), t1.get(f"base_model.model.{name}.lora_B.weight")
        r = {"q_proj": 4, "v_proj": 8, "o_proj": 8}[leaf]                 # ranks padded per layer
        assert bank.r == r and bank.A.shape == (2, r, mod.in_features) and bank.B.shape == (2, mod.out_features, r)
        if a0 is not None:
            assert torch.equal(bank.A[0, :4], a0) and torch.equal(bank.B[0, :, :4], b0)
            assert not bank.A[0, 4:].any() and not bank.B[0, :, 4:].any()     # the zero padding
            assert float(bank.scaling[0]) == 2.0
        else:                                                                 # a zero entry
            assert not bank.A[0].any() and not bank.B[0].any() and float(bank.scaling[0]) == 0.0
        if a1 is not None:
            assert torch.equal(bank.A[1], a1) and torch.equal(bank.B[1], b1) and float(bank.scaling[1]) == 1.0
        else:
            assert not bank.A[1].any() and not bank.B[1].any() and float(bank.scaling[1]) == 0.0
    assert seen == 6
    assert unload_lora_adapter(model) == 6
    assert all(m.adapter_bank is None for m in model.modules() if isinstance(m, Linear4bit))
    # a caller's slots tensor is taken as it is
    mine = torch.zeros(4, dtype=torch.int32)
    assert load_lora_adapters(model, [d0], slots=mine) is mine
    assert model.model.layers[0].self_attn.q_proj.adapter_bank.slots is mine
    with pytest.raises(ValueError, match="slots"):
        load_lora_adapters(_model(), [d0], slots=torch.zeros(4, dtype=torch.int64))


@pytest.mark.parametrize("field,value", [("use_dora", True), ("alpha_pattern", {"q_proj": 4}), ("bias", "all"),
                                         ("modules_to_save", ["lm_head"])])
def test_loader_refusals_apply_per_directory(tmp_path, field, value):
    from quantizations_amd import Linear4bit
    from quantizations_amd.integration import load_lora_adapters

    model = _model()
    good, bad = str(tmp_path / "good"), str(tmp_path / "bad")
    _write_adapter(good, model)
    _write_adapter(bad, model, **{field: value})
    with pytest.raises(NotImplementedError, match=field):
        load_lora_adapters(model, [good, bad])
    assert all(m.adapter_bank is None for m in model.modules() if isinstance(m, Linear4bit))   # nothing was set
    extra = {"base_model.model.model.layers.7.self_attn.q_proj.lora_A.weight": torch.zeros(4, 64).half(),
             "base_model.model.model.layers.7.self_attn.q_proj.lora_B.weight": torch.zeros(64, 4).half()}
    _write_adapter(bad, model, extra_keys=extra)
    with pytest.raises(KeyError, match="layers.7"):
        load_lora_adapters(model, [good, bad])
    assert all(m.adapter_bank is None for m in model.modules() if isinstance(m, Linear4bit))


def test_replace_lora_adapter_and_its_errors(tmp_path):
    from quantizations_amd.integration import load_lora_adapters, replace_lora_adapter

    model = _model()
    d0, d1, d2, d3, d4 = (str(tmp_path / f"a{i}") for i in range(5))
    _write_adapter(d0, model, targets=QV, r=8)
    _write_adapter(d1, model, targets=QV, r=4)
    load_lora_adapters(model, [d0, d1])
    q = model.model.layers[0].self_attn.q_proj
    v = model.model.layers[0].self_attn.v_proj
    ptrs = (q.adapter_bank.A.data_ptr(), q.adapter_bank.B.data_ptr(), q.adapter_bank.scaling.data_ptr())
    keep = q.adapter_bank.A[0].clone()
    # a smaller rank, on q only: written in place, padded; v (not targeted) gets a zero entry
    t2 = _write_adapter(d2, model, targets=("q_proj",), r=2)
    assert replace_lora_adapter(model, 1, d2) == 4
    bank = q.adapter_bank
    assert (bank.A.data_ptr(), bank.B.data_ptr(), bank.scaling.data_ptr()) == ptrs
    assert torch.equal(bank.A[1, :2], t2["base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight"])
    assert not bank.A[1, 2:].any() and not bank.B[1, :, 2:].any() and float(bank.scaling[1]) == 4.0
    assert torch.equal(bank.A[0], keep)
    assert not v.adapter_bank.A[1].any() and not v.adapter_bank.B[1].any() and float(v.adapter_bank.scaling[1]) == 0.0
    # a rank above the bank's: ValueError, nothing written
    _write_adapter(d3, model, targets=QV, r=16)
    before = bank.A.clone()
    with pytest.raises(ValueError, match="rank"):
        replace_lora_adapter(model, 0, d3)
    assert torch.equal(bank.A, before)
    # a targeted layer without a bank: KeyError
    _write_adapter(d4, model, targets=("q_proj", "o_proj"), r=4)
    with pytest.raises(KeyError, match="o_proj"):
        replace_lora_adapter(model, 0, d4)
    with pytest.raises(IndexError):
        replace_lora_adapter(model, 2, d1)
    assert torch.equal(bank.A, before)


def test_bank_put_pads_and_refuses_a_larger_rank():
    from quantizations_amd.lora import AdapterBank

    slots = torch.full((16,), -1, dtype=torch.int32)
    (A4, B4), (A8, B8) = _ab(4), _ab(8)
    bank = AdapterBank([(A4, B4, 0.5), None, (A8, B8, 2.0)], slots, 32, 64, torch.device("cpu"))
    assert (bank.n, bank.r) == (3, 8) and bank.slots is slots
    assert torch.equal(bank.A[0, :4], A4) and not bank.A[0, 4:].any() and not bank.A[1].any()
    assert bank.scaling.tolist() == [0.5, 0.0, 2.0]
    bank.put(2, A4, B4, 1.5)                                      # a smaller rank over a larger one: re-padded
    assert torch.equal(bank.B[2, :, :4], B4) and not bank.B[2, :, 4:].any() and not bank.A[2, 4:].any()
    bank.put(0)                                                    # a zero entry
    assert not bank.A[0].any() and float(bank.scaling[0]) == 0.0
    A16, B16 = _ab(16)
    with pytest.raises(ValueError, match="rank"):
        bank.put(1, A16, B16, 1.0)
    with pytest.raises(IndexError):
        bank.put(3, A4, B4, 1.0)
    with pytest.raises(ValueError):
        AdapterBank([None, None], slots, 32, 64, torch.device("cpu"))
    with pytest.raises(ValueError):
        AdapterBank([(A4, B4, 1.0)], slots.long(), 32, 64, torch.device("cpu"))


def test_adapter_and_bank_are_exclusive():
    import quantizations_amd as qa

    lin = qa.Linear4bit(64, 32, quant_type="nf4")
    A, B = _ab(4)
    slots = torch.zeros(16, dtype=torch.int32)
    lin.set_adapter(A, B, 1.0)
    with pytest.raises(ValueError, match="adapter"):
        lin.set_adapter_bank([(A, B, 1.0)], slots)
    assert lin.adapter_bank is None
    lin.clear_adapter()
    lin.set_adapter_bank([(A, B, 1.0)], slots)
    with pytest.raises(ValueError, match="bank"):
        lin.set_adapter(A, B, 1.0)
    assert lin.adapter is None and lin.adapter_bank is not None
    lin.clear_adapter_bank()
    lin.clear_adapter_bank()                                      # idempotent
    lin.set_adapter(A, B, 1.0)


def test_bank_not_in_state_dict_and_kept_by_deepcopy():
    import quantizations_amd as qa

    lin = qa.Linear4bit(64, 32, bias=True, quant_type="nf4")
    keys = list(lin.state_dict().keys())
    A, B = _ab(4)
    slots = torch.tensor([1, -1, 0], dtype=torch.int32)
    lin.set_adapter_bank([None, (A, B, 0.5)], slots)
    assert list(lin.state_dict().keys()) == keys
    assert lin.adapter_bank.A.data_ptr() != A.data_ptr()          # its own buffers
    holder = torch.nn.ModuleList([lin, qa.Linear4bit(64, 32, quant_type="nf4")])
    holder[1].set_adapter_bank([(A, B, 1.0), None], slots)
    cp = copy.deepcopy(holder)
    b0, b1 = cp[0].adapter_bank, cp[1].adapter_bank
    assert b0 is not lin.adapter_bank and torch.equal(b0.A, lin.adapter_bank.A) and torch.equal(b0.B, lin.adapter_bank.B)
    assert torch.equal(b0.scaling, lin.adapter_bank.scaling) and b0.A.data_ptr() != lin.adapter_bank.A.data_ptr()
    assert torch.equal(b0.slots, slots) and b0.slots is not slots and b0.slots is b1.slots    # still one shared tensor
    lin.clear_adapter_bank()
    assert lin.adapter_bank is None and cp[0].adapter_bank is not None


def test_sharding_refuses_a_layer_with_a_bank():
    from quantizations_amd.parallel import apply_tensor_parallel, shard_model_linear4bit

    slots = torch.zeros(16, dtype=torch.int32)
    ent = [(torch.zeros(4, 64).half(), torch.zeros(64, 4).half(), 1.0)]
    model = _model()
    model.model.layers[0].self_attn.q_proj.set_adapter_bank(ent, slots)
    with pytest.raises(NotImplementedError, match="bank"):
        shard_model_linear4bit(model, rank=0, world_size=2)
    model = _model()
    model.model.layers[0].self_attn.o_proj.set_adapter_bank(ent, slots)
    with pytest.raises(NotImplementedError, match="bank"):
        apply_tensor_parallel(model, rank=0, world_size=2)


def test_too_many_streams_raises_and_rows_map_to_streams():
    from quantizations_amd import lora

    A, B = _ab(4)
    bank = lora.AdapterBank([(A, B, 1.0)], torch.zeros(4, dtype=torch.int32), 32, 64, torch.device("cpu"))
    assert lora.bank_rows(bank, torch.zeros(4, 1, 64)) == (4, 1)            # [B, 1, K] decode
    assert lora.bank_rows(bank, torch.zeros(4, 3, 64)) == (12, 3)           # [B, S, K] prefill
    assert lora.bank_rows(bank, torch.zeros(4, 64)) == (4, 1)               # 2-D: one row per stream
    assert lora.bank_rows(bank, torch.zeros(2, 2, 5, 64)) == (20, 5)
    for shape in [(5, 1, 64), (5, 64), (5, 3, 64)]:
        with pytest.raises(ValueError, match="streams"):
            lora.bank_rows(bank, torch.zeros(*shape))
        with pytest.raises(ValueError, match="streams"):
            lora.composed_bank_term(bank, torch.zeros(*shape), torch.float32)


def test_composed_bank_term_on_the_cpu():
    """The composed route against the per-row definition (fp32, CPU): slots -1, out-of-range values,
    S rows per stream, and a bank without slots (every row on entry 0)."""
    from quantizations_amd import lora

    g = torch.Generator().manual_seed(3)
    ents = [(torch.randn(r, 64, generator=g), torch.randn(32, r, generator=g), s) for r, s in ((4, 1.0), (2, 0.5), (8, 2.0))]
    slots = torch.tensor([2, -1, 0, 3, 1, 99, -7, 0], dtype=torch.int32)
    bank = lora.AdapterBank(ents, slots, 32, 64, torch.device("cpu"))
    for shape, S in [((5, 1, 64), 1), ((4, 3, 64), 3), ((7, 64), 1), ((1, 1, 64), 1)]:
        x = torch.randn(*shape, generator=g)
        got = lora.composed_bank_term(bank, x, torch.float32).reshape(-1, 32)
        rows = x.reshape(-1, 64)
        for c in range(rows.shape[0]):
            a = int(slots[c // S])
            want = torch.zeros(32) if not 0 <= a < 3 else ents[a][2] * (ents[a][1] @ (ents[a][0] @ rows[c]))
            assert torch.allclose(got[c], want, rtol=1e-5, atol=1e-5), (shape, c)
            if not 0 <= a < 3:
                assert not got[c].any()
    bank.set_slots(None)
    x = torch.randn(3, 64, generator=g)
    want = ents[0][2] * (x @ ents[0][0].T @ ents[0][1].T)
    assert torch.allclose(lora.composed_bank_term(bank, x, torch.float32), want, rtol=1e-5, atol=1e-5)
