"""-m "not gpu": element-wise dropout of the finetuning model (include/memhip.h, memhip_dropout_t): the mask contract restated
in numpy (Philox4x32-10 known-answer vector), the model surface (state dict, Dropout sites, refusals) and the ISA of the
gemm_p8 residual-dropout kernel."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 on uint64 numpy arrays holding uint32 values: ctr = (c0, c1, c2, c3) arrays, key = (k0, k1) scalars."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in ctr)
    k0, k1 = np.uint64(key[0] & M32), np.uint64(key[1] & M32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(M32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(M32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(0x9E3779B9)) & np.uint64(M32)
        k1 = (k1 + np.uint64(0xBB67AE85)) & np.uint64(M32)
    return c0, c1, c2, c3


def keep_mask(key0, key1, site, p, row0, rows, cols):
    """The mask contract of memhip.h: u8 [rows, cols] keep bits of residual-stream rows row0 .. row0 + rows - 1."""
    thr = int(round(p * 65536))
    r = np.arange(row0, row0 + rows, dtype=np.uint64)[:, None]
    g = np.arange(cols // 8, dtype=np.uint64)[None, :]
    r, g = np.broadcast_arrays(r, g)
    w = philox4x32_10((r, g, np.full_like(r, site), np.zeros_like(r)), (key0, key1))
    halves = []
    for j in range(8):
        halves.append((w[j >> 1] >> np.uint64(16 * (j & 1))) & np.uint64(0xFFFF))
    h = np.stack(halves, -1).reshape(rows, cols)
    return (h >= thr).astype(np.uint8)


def test_philox_known_answer():
    """Random123's philox4x32_10 known-answer vector (key 0, counter 0), which at::Philox4_32 also produces."""
    w = philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(x) for x in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    # the second Random123 vector: all ones
    w = philox4x32_10((M32, M32, M32, M32), (M32, M32))
    assert [int(x) for x in w] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_mask_contract_law():
    """Keep rate 1 - thr / 65536 within 5 sigma; p = 0 keeps everything; sites and rows give different masks."""
    for p in (0.1, 0.5):
        m = keep_mask(123, 456, 3, p, 0, 512, 768)
        q = 1.0 - round(p * 65536) / 65536
        n = m.size
        assert abs(m.mean() - q) <= 5 * np.sqrt(q * (1 - q) / n), (p, m.mean())
    assert keep_mask(1, 2, 0, 0.0, 0, 64, 64).all()
    a, b = keep_mask(7, 8, 0, 0.5, 0, 64, 64), keep_mask(7, 8, 1, 0.5, 0, 64, 64)
    assert (a != b).mean() > 0.4
    assert np.array_equal(keep_mask(7, 8, 0, 0.5, 10, 54, 64), a[10:])


def test_finetune_model_builds_with_dropout():
    """ft_vit(drop_rate=0.1): the reference's module tree (same state dict) with nn.Dropout(0.1) at pos_drop, every
    Attention.proj_drop and Mlp.drop; attn_drop stays 0."""
    from mem_amd.modeling_finetune import ft_vit
    from oracle.gen_golden_ft import FT_A
    m0, m1 = ft_vit(**FT_A), ft_vit(**dict(FT_A, drop_rate=0.1))
    s0, s1 = m0.state_dict(), m1.state_dict()
    assert list(s0.keys()) == list(s1.keys())
    assert all(s0[k].shape == s1[k].shape for k in s0)
    assert m1.pos_drop.p == 0.1 and m1.drop_rate == 0.1
    for blk in m1.blocks:
        assert blk.attn.proj_drop.p == 0.1 and blk.mlp.drop.p == 0.1 and blk.attn.attn_drop.p == 0.0
    assert m0.draw_dropout_key() is None


def test_dropout_refusals():
    from mem_amd.modeling_finetune import ft_vit
    from mem_amd.modeling_pretrain import pt_vit
    from oracle.gen_golden_ft import FT_A
    with pytest.raises(AssertionError, match="attn_drop_rate"):
        ft_vit(**dict(FT_A, attn_drop_rate=0.1))
    with pytest.raises(AssertionError):
        pt_vit(img_size=64, patch_size=16, in_chans=2, embed_dim=128, depth=1, num_heads=2, vocab_size=64, drop_rate=0.1)
    from mem_amd.vit_engine_f32 import ViTEngineF32
    with pytest.raises(AssertionError, match="fp32 parity"):
        ViTEngineF32(ft_vit(**dict(FT_A, drop_rate=0.1)))


def test_dropout_key_draw_is_reproducible():
    """The key comes from the model's drop-path stream: restoring its state reproduces it."""
    from mem_amd.modeling_finetune import ft_vit
    from oracle.gen_golden_ft import FT_A
    m = ft_vit(**dict(FT_A, drop_rate=0.1))
    from mem_amd.utils import DropPathStream
    m._dp_stream = DropPathStream()
    m._dp_stream.seed(17)
    st = m._dp_stream.state()
    k1 = m.draw_dropout_key()
    k2 = m.draw_dropout_key()
    m._dp_stream.load_state(st)
    assert m.draw_dropout_key() == k1 and k1 != k2
    assert all(0 <= k < (1 << 32) for k in k1)


def _kernel_body(lines, name):
    i0 = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and name in l.split(":")[0])
    j = i0
    while not lines[j].startswith(".Lfunc_end"):          # (the whole function: the paired kernel ends twice)
        j += 1
    return lines[i0:j]


def test_gemm_p8_residual_dropout_epilogue_isa(tmp_path):
    """The residual-dropout instantiations of gemm_p8 (128-row tiles, with and without the row guard: the form every
    dropout product of gemm_p8 runs on) do not spill -- a spill would add vector-memory operations behind the main loop's
    counted LDS-DMA waits -- and there is no 256-row dropout form (its hand-counted residual-row waits leave no room for the
    Philox state).  The existing instantiations are checked by test_abi.py."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "mem_amd", "csrc", "gemm_p8.hip")
    out = str(tmp_path / "gemm_p8.s")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-fast-math", "-w", "-S",
                    "--cuda-device-only", "-o", out, src], check=True, capture_output=True)
    lines = open(out).read().split("\n")
    names = sorted({m.group(1) for l in lines for m in [re.match(r"^(_Z\w*drop\w*):", l)] if m})
    assert any("gemm_p8_drop_kernelILi128ELb0E" in n for n in names) and any("gemm_p8_drop_kernelILi128ELb1E" in n for n in names), names
    assert not any("ILi256E" in n for n in names), names
    for n in names:
        body = _kernel_body(lines, n)
        assert not any("scratch_" in l for l in body), n
        assert any("v_mul_hi_u32" in l for l in body), n          # the Philox rounds are there
