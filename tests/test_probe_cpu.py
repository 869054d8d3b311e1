"""-m "not gpu": the host side of frozen-backbone probing -- the token-pooling entry points are exported and validate their
arguments before any launch, the stage-3 parser accepts --freeze_backbone, and freeze_backbone() on a CPU-constructed ft_vit
leaves exactly the head trainable (no engine is touched)."""
import contextlib
import io

import pytest

TINY = dict(img_size=(32, 48), patch_size=(16, 16), in_chans=3, num_classes=5, embed_dim=64, depth=2, num_heads=1, mlp_ratio=4,
            drop_path_rate=0.1, init_values=0.1, use_abs_pos_emb=False, use_rel_pos_bias=True, use_mean_pooling=True)


def _lib():
    from mem_amd import _lib, ops  # noqa: F401  (ops declares the signatures)
    return _lib.lib


def _bad(rc, lib, word):
    assert rc == -1, rc
    assert word.encode() in lib.memhip_last_error(), lib.memhip_last_error()


def test_pool_symbols_are_exported_and_the_abi_number_stays():
    lib = _lib()
    assert lib.memhip_abi_version() == 10                                       # (7 when these symbols came, additively; 8: the struct entry points; 9: the tokenizer's args struct; 10: the rasterizer's)
    for name in ("memhip_pool_tokens", "memhip_pool_tokens_bwd"):
        assert hasattr(lib, name), name


def test_pool_entries_validate_before_any_launch():
    """Null pointers and bad shapes return MEMHIP_EINVAL with a message; nothing is launched (no GPU here)."""
    import ctypes as C
    import numpy as np
    lib = _lib()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    # memhip_pool_tokens(x, ldx, B, T, D, out, stream)
    _bad(lib.memhip_pool_tokens(None, 8, 2, 4, 8, None, None), lib, "null pointer")
    _bad(lib.memhip_pool_tokens(p, 8, 2, 4, 8, None, None), lib, "null pointer")
    _bad(lib.memhip_pool_tokens(p, 8, 2, 1, 8, p, None), lib, "bad shape")      # T < 2: no token behind the cls row
    _bad(lib.memhip_pool_tokens(p, 8, 2, 4, 0, p, None), lib, "bad shape")      # D <= 0
    _bad(lib.memhip_pool_tokens(p, 8, 0, 4, 8, p, None), lib, "bad shape")
    _bad(lib.memhip_pool_tokens(p, 4, 2, 4, 8, p, None), lib, "ldx=")           # ldx < D
    # memhip_pool_tokens_bwd(dout, B, T, D, dx, stream)
    _bad(lib.memhip_pool_tokens_bwd(None, 2, 4, 8, None, None), lib, "null pointer")
    _bad(lib.memhip_pool_tokens_bwd(p, 2, 4, 8, None, None), lib, "null pointer")
    _bad(lib.memhip_pool_tokens_bwd(p, 2, 1, 8, p, None), lib, "bad shape")
    _bad(lib.memhip_pool_tokens_bwd(p, 2, 4, -1, p, None), lib, "bad shape")


def test_get_args_accepts_freeze_backbone_and_still_refuses_linear_probe():
    from mem_amd.run_class_finetuning import REFUSED, get_args
    a = get_args(["--expweek", "x", "--freeze_backbone", "1"])
    assert a.freeze_backbone == 1
    assert get_args(["--expweek", "x"]).freeze_backbone == 0
    assert "freeze_backbone" not in REFUSED
    with pytest.raises(NotImplementedError) as e:
        get_args(["--expweek", "x", "--freeze_backbone", "1", "--linear_probe"])
    msg = str(e.value)
    assert msg.startswith("--linear_probe") and "freeze_backbone" not in msg and "\n" not in msg, msg


def test_freeze_backbone_leaves_exactly_the_head_trainable():
    from mem_amd import optim_factory as OF
    from mem_amd.modeling_finetune import ft_vit
    m = ft_vit(**TINY)
    assert not m._trunk_frozen()
    names = [n for n, _ in m.named_parameters()]
    frozen = m.freeze_backbone()
    assert m._engine is None                                                      # nothing touched the GPU engine
    kept = [n for n, p in m.named_parameters() if p.requires_grad]
    assert kept and all(n.startswith(("head.", "fc_norm.")) for n in kept)
    assert sorted(kept) == sorted(n for n in names if n.startswith(("head.", "fc_norm.")))
    assert sorted(frozen + kept) == sorted(names) and not set(frozen) & set(kept)
    assert m._trunk_frozen() and m.training                                      # still train(): drop path / dropout act
    depth = TINY["depth"]
    assigner = OF.LayerDecayValueAssigner([0.75 ** (depth + 1 - i) for i in range(depth + 2)])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        groups = OF.get_parameter_groups(m, 0.05, m.no_weight_decay(), assigner.get_layer_id, assigner.get_scale)
    got = {id(p) for g in groups for p in g["params"]}
    assert got == {id(p) for n, p in m.named_parameters() if n in kept}
    assert all(g["lr_scale"] == 1.0 for g in groups)                              # the head is the last layer id
    assert "blocks." not in out.getvalue() and "patch_embed" not in out.getvalue()


def test_cls_form_freezes_its_final_norm_with_the_trunk():
    from mem_amd.modeling_finetune import ft_vit
    m = ft_vit(**dict(TINY, use_mean_pooling=False))
    m.freeze_backbone()
    kept = [n for n, p in m.named_parameters() if p.requires_grad]
    assert sorted(kept) == ["head.bias", "head.weight"] and m._trunk_frozen()
