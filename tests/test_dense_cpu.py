"""-m "not gpu": the host side of the dense per-block feature maps -- the two entry points are declared, exported and bound and
validate their arguments before any launch, forward_dense validates out_indices before it touches a device, and the
segmentation backbone carries the reference's state-dict keys (necks: written down from the reference's module structure,
mem/semantic_segmentation/backbone/mem.py:331-346; trunk: ft_vit's keys without head and fc_norm)."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(img_size=(32, 48), patch_size=(16, 16), in_chans=3, embed_dim=64, depth=6, num_heads=1, mlp_ratio=4,
             drop_path_rate=0.1, init_values=0.1, use_abs_pos_emb=False, use_rel_pos_bias=True)

# ConvTranspose2d, SyncBatchNorm, GELU, ConvTranspose2d | ConvTranspose2d | Identity | MaxPool2d
FPN_KEYS = ["fpn1.0.weight", "fpn1.0.bias", "fpn1.1.weight", "fpn1.1.bias", "fpn1.1.running_mean", "fpn1.1.running_var",
            "fpn1.1.num_batches_tracked", "fpn1.3.weight", "fpn1.3.bias", "fpn2.0.weight", "fpn2.0.bias"]


def _lib():
    from mem_amd import _lib, ops  # noqa: F401  (ops declares the signatures)
    return _lib.lib


def _bad(rc, lib, word):
    assert rc == -1, rc
    assert word.encode() in lib.memhip_last_error(), lib.memhip_last_error()


def test_dense_symbols_are_declared_exported_and_bound():
    lib = _lib()
    from mem_amd import ops
    header = open(os.path.join(ROOT, "include", "memhip.h")).read()
    assert lib.memhip_abi_version() == 10                                       # (7 when these symbols came, additively; 8: the struct entry points; 9: the tokenizer's args struct; 10: the rasterizer's)
    for name in ("memhip_tokens_to_maps", "memhip_maps_to_tokens_add"):
        assert f"int {name}(" in header, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name                    # ops.py declared its signature
    assert callable(ops.tokens_to_maps) and callable(ops.maps_to_tokens_add)


def test_dense_entries_validate_before_any_launch():
    """D % 64 != 0, T < 2, a leading dimension below D and null pointers return MEMHIP_EINVAL with a message; nothing is
    launched (no GPU here)."""
    import ctypes as C
    import numpy as np
    lib = _lib()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    # memhip_tokens_to_maps(x, ldx, b0, b1, T, D, out, stream)
    _bad(lib.memhip_tokens_to_maps(p, 96, 0, 2, 5, 96, p, None), lib, "bad shape")       # D % 64 != 0
    _bad(lib.memhip_tokens_to_maps(p, 64, 0, 2, 1, 64, p, None), lib, "bad shape")       # T < 2
    _bad(lib.memhip_tokens_to_maps(p, 32, 0, 2, 5, 64, p, None), lib, "ldx=")            # ldx < D
    _bad(lib.memhip_tokens_to_maps(p, 64, 2, 2, 5, 64, p, None), lib, "sample range")    # empty range
    _bad(lib.memhip_tokens_to_maps(None, 64, 0, 2, 5, 64, p, None), lib, "null pointer")
    _bad(lib.memhip_tokens_to_maps(p, 64, 0, 2, 5, 64, None, None), lib, "null pointer")
    # memhip_maps_to_tokens_add(dmap, b0, b1, T, D, dx, lddx, stream)
    _bad(lib.memhip_maps_to_tokens_add(p, 0, 2, 5, 96, p, 96, None), lib, "bad shape")
    _bad(lib.memhip_maps_to_tokens_add(p, 0, 2, 1, 64, p, 64, None), lib, "bad shape")
    _bad(lib.memhip_maps_to_tokens_add(p, 0, 2, 5, 64, p, 32, None), lib, "lddx=")
    _bad(lib.memhip_maps_to_tokens_add(p, 1, 0, 5, 64, p, 64, None), lib, "sample range")
    _bad(lib.memhip_maps_to_tokens_add(None, 0, 2, 5, 64, p, 64, None), lib, "null pointer")
    _bad(lib.memhip_maps_to_tokens_add(p, 0, 2, 5, 64, None, 64, None), lib, "null pointer")


@pytest.mark.parametrize("bad,word", [((5, 3), "ascend, 3 follows 5"), ((3, 3), "index 3 given twice"), ((6,), "index 6 outside"),
                                      ((-1, 2), "index -1 outside"), ((), "no block")])
def test_forward_dense_rejects_bad_out_indices_on_the_host(bad, word):
    import torch
    from mem_amd.modeling_finetune import ft_vit
    m = ft_vit(num_classes=3, use_mean_pooling=True, **SMALL)
    assert len(m.blocks) == 6
    with pytest.raises(ValueError) as e:
        m.forward_dense(torch.zeros(1, 3, 32, 48), out_indices=bad)
    assert word in str(e.value), str(e.value)
    assert m._engine is None                                                    # nothing touched the GPU engine


def test_evbeit_state_dict_keys():
    from mem_amd.modeling_finetune import ft_vit
    from mem_amd.semseg_backbone import EvBEiT
    m = EvBEiT(out_indices=(1, 2, 3, 5), **SMALL)
    keys = list(m.state_dict().keys())
    assert [k for k in keys if k.startswith("fpn")] == FPN_KEYS
    ft = ft_vit(num_classes=3, use_mean_pooling=True, **SMALL)
    want = [k for k in ft.state_dict().keys() if not k.startswith(("head.", "fc_norm."))]
    assert [k for k in keys if not k.startswith("fpn")] == want
    assert m._engine is None
    ref = ft.state_dict()
    assert all(m.state_dict()[k].shape == ref[k].shape for k in want)


def test_evbeit_refuses_what_it_does_not_mirror():
    from mem_amd.semseg_backbone import EvBEiT
    with pytest.raises(NotImplementedError) as e:
        EvBEiT(use_checkpoint=False, **SMALL)
    assert "use_checkpoint" in str(e.value)
    with pytest.raises(NotImplementedError):
        EvBEiT(**dict(SMALL, patch_size=(8, 8)))
    with pytest.raises(ValueError):
        EvBEiT(out_indices=(1, 2, 3), **SMALL)
    with pytest.raises(ValueError):
        EvBEiT(out_indices=(1, 2, 3, 6), **SMALL)
