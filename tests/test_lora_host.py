"""CPU: the LoRA adapter API of Linear4bit (set_adapter / clear_adapter / adapter), the peft adapter
directory loader (integration.load_lora_adapter) and the sharding functions' refusal, on a tiny
random-init Llama whose Linear4bit layers were never moved to a GPU (no kernel runs)."""
import copy
import json
import math
import os

import pytest
import torch


def _model():
    from transformers import LlamaConfig, LlamaForCausalLM

    from quantizations_amd.integration import replace_with_bnb_linear

    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=64)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).half().eval()
    replace_with_bnb_linear(model, quant_type="nf4", compute_dtype=torch.float16)
    return model


def _write_adapter(path, model, targets=("q_proj", "v_proj"), r=4, ranks=None, extra_keys=None, **cfg):
    """A peft adapter directory for `model`: lora_A / lora_B of rank r (ranks: {module path: rank}) on
    every module whose name ends in one of `targets`."""
    from safetensors.torch import save_file

    g = torch.Generator().manual_seed(1)
    tensors = {}
    for name, mod in model.named_modules():
        if name.split(".")[-1] in targets and hasattr(mod, "in_features"):
            rr = (ranks or {}).get(name, r)
            tensors[f"base_model.model.{name}.lora_A.weight"] = torch.randn(rr, mod.in_features, generator=g).half()
            tensors[f"base_model.model.{name}.lora_B.weight"] = torch.randn(mod.out_features, rr, generator=g).half()
    tensors.update(extra_keys or {})
    os.makedirs(path, exist_ok=True)
    save_file(tensors, os.path.join(path, "adapter_model.safetensors"))
    conf = {"peft_type": "LORA", "r": r, "lora_alpha": 8, "use_rslora": False, "target_modules": list(targets),
            "bias": "none", "use_dora": False, "alpha_pattern": {}, "rank_pattern": {}, "modules_to_save": None}
    conf.update(cfg)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(conf, f)
    return tensors


def test_loader_maps_keys_and_scaling(tmp_path):
    from quantizations_amd import Linear4bit
    from quantizations_amd.integration import load_lora_adapter, unload_lora_adapter

    model = _model()
    tensors = _write_adapter(str(tmp_path), model, r=4)
    assert load_lora_adapter(model, str(tmp_path)) == 4          # q and v of two layers
    for name, mod in model.named_modules():
        if not isinstance(mod, Linear4bit):
            continue
        if name.split(".")[-1] in ("q_proj", "v_proj"):
            ad = mod.adapter
            assert torch.equal(ad.A, tensors[f"base_model.model.{name}.lora_A.weight"])
            assert torch.equal(ad.B, tensors[f"base_model.model.{name}.lora_B.weight"])
            assert ad.A.is_contiguous() and ad.B.is_contiguous() and ad.A.device == mod.weight.device
            assert ad.scaling.dtype == torch.float32 and ad.scaling.numel() == 1
            assert float(ad.scaling) == 8 / 4
        else:
            assert mod.adapter is None
    assert unload_lora_adapter(model) == 4
    assert all(m.adapter is None for m in model.modules() if isinstance(m, Linear4bit))


def test_loader_rslora_and_rank_from_shapes(tmp_path):
    from quantizations_amd.integration import load_lora_adapter

    model = _model()
    odd = "model.layers.1.self_attn.v_proj"
    _write_adapter(str(tmp_path), model, r=4, ranks={odd: 16}, use_rslora=True, rank_pattern={odd: 16})
    load_lora_adapter(model, str(tmp_path))
    mods = dict(model.named_modules())
    assert mods[odd].adapter.r == 16
    assert float(mods[odd].adapter.scaling) == pytest.approx(8 / math.sqrt(16), rel=1e-7)
    q = mods["model.layers.0.self_attn.q_proj"].adapter
    assert q.r == 4 and float(q.scaling) == pytest.approx(8 / math.sqrt(4), rel=1e-7)
    # plain LoRA with the rank from the shapes: alpha / 16, not alpha / cfg.r
    _write_adapter(str(tmp_path), model, r=4, ranks={odd: 16})
    load_lora_adapter(model, str(tmp_path))
    assert float(mods[odd].adapter.scaling) == 8 / 16


@pytest.mark.parametrize("field,value", [("use_dora", True), ("alpha_pattern", {"q_proj": 4}), ("bias", "all"),
                                         ("bias", "lora_only"), ("modules_to_save", ["lm_head"])])
def test_loader_rejects_config_fields(tmp_path, field, value):
    from quantizations_amd import Linear4bit
    from quantizations_amd.integration import load_lora_adapter

    model = _model()
    _write_adapter(str(tmp_path), model, **{field: value})
    with pytest.raises(NotImplementedError, match=field):
        load_lora_adapter(model, str(tmp_path))
    assert all(m.adapter is None for m in model.modules() if isinstance(m, Linear4bit))


def test_loader_unknown_module_key(tmp_path):
    from quantizations_amd import Linear4bit
    from quantizations_amd.integration import load_lora_adapter

    model = _model()
    extra = {"base_model.model.model.layers.7.self_attn.q_proj.lora_A.weight": torch.zeros(4, 64).half(),
             "base_model.model.model.layers.7.self_attn.q_proj.lora_B.weight": torch.zeros(64, 4).half()}
    _write_adapter(str(tmp_path), model, extra_keys=extra)
    with pytest.raises(KeyError, match="layers.7"):
        load_lora_adapter(model, str(tmp_path))
    assert all(m.adapter is None for m in model.modules() if isinstance(m, Linear4bit))
    # lm_head stays an nn.Linear (not converted): not a Linear4bit of the model
    extra = {"base_model.model.lm_head.lora_A.weight": torch.zeros(4, 64).half(),
             "base_model.model.lm_head.lora_B.weight": torch.zeros(64, 4).half()}
    _write_adapter(str(tmp_path), model, targets=("q_proj", "v_proj", "lm_head"), extra_keys=extra)
    with pytest.raises(KeyError, match="lm_head"):
        load_lora_adapter(model, str(tmp_path))


def test_adapter_not_in_state_dict_kept_by_deepcopy_and_cleared():
    import quantizations_amd as qa

    lin = qa.Linear4bit(64, 32, bias=True, quant_type="nf4")
    keys = list(lin.state_dict().keys())
    A, B = torch.randn(4, 64).half(), torch.randn(32, 4).half()
    lin.set_adapter(A, B, 0.5)
    assert list(lin.state_dict().keys()) == keys
    ad = lin.adapter
    assert torch.equal(ad.A, A) and torch.equal(ad.B, B) and float(ad.scaling) == 0.5
    assert ad.A.data_ptr() != A.data_ptr()                        # its own buffers
    # same shapes and dtype: copied in place into the buffers a captured graph reads
    pa, pb, ps = ad.A.data_ptr(), ad.B.data_ptr(), ad.scaling.data_ptr()
    lin.set_adapter(A * 2, B * 3, 0.25)
    assert lin.adapter is ad and (ad.A.data_ptr(), ad.B.data_ptr(), ad.scaling.data_ptr()) == (pa, pb, ps)
    assert torch.equal(ad.A, A * 2) and torch.equal(ad.B, B * 3) and float(ad.scaling) == 0.25
    # another rank: new buffers
    lin.set_adapter(torch.randn(8, 64).half(), torch.randn(32, 8).half(), 1.0)
    assert lin.adapter is not ad and lin.adapter.r == 8
    cp = copy.deepcopy(lin)
    assert cp.adapter is not None and cp.adapter is not lin.adapter
    assert torch.equal(cp.adapter.A, lin.adapter.A) and torch.equal(cp.adapter.B, lin.adapter.B)
    assert torch.equal(cp.adapter.scaling, lin.adapter.scaling)
    assert cp.adapter.A.data_ptr() != lin.adapter.A.data_ptr()
    lin.clear_adapter()
    assert lin.adapter is None and cp.adapter is not None
    lin.clear_adapter()                                           # idempotent
    with pytest.raises(ValueError):
        lin.set_adapter(torch.randn(4, 63).half(), B, 1.0)        # K mismatch
    with pytest.raises(ValueError):
        lin.set_adapter(A, torch.randn(32, 5).half(), 1.0)        # rank mismatch


def test_sharding_refuses_a_layer_with_an_adapter():
    from quantizations_amd.parallel import apply_tensor_parallel, shard_model_linear4bit

    model = _model()
    q = model.model.layers[0].self_attn.q_proj
    q.set_adapter(torch.zeros(4, 64).half(), torch.zeros(64, 4).half(), 1.0)
    with pytest.raises(NotImplementedError, match="adapter"):
        shard_model_linear4bit(model, rank=0, world_size=2)
    model = _model()
    model.model.layers[0].self_attn.o_proj.set_adapter(torch.zeros(4, 64).half(), torch.zeros(64, 4).half(), 1.0)
    with pytest.raises(NotImplementedError, match="adapter"):
        apply_tensor_parallel(model, rank=0, world_size=2)
