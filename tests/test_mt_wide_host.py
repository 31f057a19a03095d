"""CPU: the host side of the wide multi-token path -- the decode_rows opt-in and what it refuses."""
import inspect

import pytest
import torch


def test_set_decode_rows_sets_every_layer_and_group():
    import quantizations_amd as qa
    from quantizations_amd import core, integration
    from quantizations_amd.modules import DecodeGroup, _linear4bit_group_compute

    assert (core.MT_MAX_TOKENS, core.MT_WIDE_MAX_TOKENS) == (16, 64)
    lins = [qa.Linear4bit(256, 64, device="meta") for _ in range(3)]
    model = torch.nn.Sequential(*lins)
    grp = DecodeGroup(lins[:2], _linear4bit_group_compute)
    for m in lins[:2]:
        m.__dict__["_qz_group"] = grp
    assert grp.decode_rows == 16 and all(m.decode_rows == 16 for m in lins)
    for bad in (15, 65):
        with pytest.raises(ValueError, match="16..64"):
            integration.set_decode_rows(model, bad)
    assert qa.set_decode_rows(model, 64) == 3
    assert grp.decode_rows == 64 and all(m.decode_rows == 64 for m in lins)
    # nothing on the CPU, with autograd or outside 17..64 rows is let in
    x = torch.zeros(20, 256, dtype=torch.float16)
    assert not grp.accepts_wide(x) and not core.grouped_wide_ok(x, [(None, None)])
    assert qa.set_decode_rows(model, 16) == 3 and DecodeGroup.decode_rows == 16


@pytest.mark.parametrize("name", ["SpeculativeSession", "StreamSession", "generate", "generate_ragged"])
def test_decode_rows_keyword_defaults_to_none(name):
    import quantizations_amd as qa

    fn = getattr(qa, name)
    sig = inspect.signature(fn.__init__ if inspect.isclass(fn) else fn)
    assert sig.parameters["decode_rows"].default is None
