"""What hipcc makes of the row kernels (rowops.hip) at D = 768: the wait and branch patterns of the row loop, read from the
device listing (hipcc --cuda-device-only -S with the Makefile's flags).  No GPU; skipped where hipcc is absent.

The row loop of layernorm_bwd, branch_bwd and layernorm_bwd_branch issues every load and store unconditionally, so that
its waits can be counted.  For the D = 768 instantiations this file asserts, between the loop's header and its back-edge:
  * no `s_waitcnt vmcnt(0)`,
  * no global / buffer load between the first and the last global store,
  * the recorded number of `s_and_saveexec` (none guards a chunk: the width fills its three chunks),
and, from the kernel descriptors, register and LDS figures at or below those of the kernels this form replaced.
layernorm_fwd has one row per wave and no row loop: the same patterns are asserted over the whole kernel, where the one
full wait is for the row's last chunk -- the last load issued, with gamma and beta requested ahead of it.
layernorm_bwd_branch has a second loop for the rows of samples that one of the two branches dropped; it runs behind
run-time conditions, keeps hipcc's worst-case waits by design, and is not the subject here: the row loop is the FIRST loop
with global stores in the listing, and the test checks that the second one is there."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mem_amd", "csrc")

# D = 768: three float4 chunks per lane, every lane owns every chunk.  name -> (mangled prefix, loops with stores, VGPRs of
# the kernel this one replaced, s_and_saveexec allowed in the row loop)
KERNELS = {
    "ln_bwd_kernel<3, full, accumulate>": ("13ln_bwd_kernelILi3ELb1ELb1EE", 1, 116, 0),
    "ln_bwd_kernel<3, full, overwrite>": ("13ln_bwd_kernelILi3ELb1ELb0EE", 1, 116, 0),
    "branch_bwd_kernel<3, full, no y>": ("17branch_bwd_kernelILi3ELb1ELb0EJEE", 1, 100, 0),
    "ln_bwd_branch_kernel<3, full, no y>": ("20ln_bwd_branch_kernelILi3ELb1ELb0EJEE", 2, 142, 0),
}
LN_FWD = ("13ln_fwd_kernelILi3ELb1EE", 58)


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def _makefile_flags():
    """CXXFLAGS of mem_amd/csrc/Makefile with ARCH and EXTRA at their defaults"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("listing") / "rowops.s")
    cmd = [hipcc] + _makefile_flags() + ["--cuda-device-only", "-S", os.path.join(CSRC, "rowops.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


_INS = re.compile(r"^\s+([a-z][a-z0-9_]+)(\s|$)")


def _kernel(text, prefix):
    """(basic blocks [(label, [instructions])], descriptor figures) of the kernel whose mangled name holds `prefix`"""
    names = [m.group(1) for m in re.finditer(r"^(_Z\w+):", text, re.M) if prefix in m.group(1)]
    assert len(names) == 1, (prefix, names)
    name = names[0]
    body = text[text.index("\n" + name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    blocks = [["entry", []]]
    for line in body.split("\n")[2:]:
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            blocks.append([m.group(1), []])
        elif _INS.match(line) and not line.lstrip().startswith((";", ".")):
            blocks[-1][1].append(line.strip())
    md = re.search(r"\.group_segment_fixed_size:\s*(\d+)(?:(?!\.group_segment_fixed_size).)*?\.name:\s+" + re.escape(name) +
                   r"\s.*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", text, re.S)
    return blocks, dict(lds=int(md.group(1)), vgpr=int(md.group(2)), spill=int(md.group(3)))


def _store_loops(blocks):
    """the loops (strongly connected sets of basic blocks) that hold global stores, each as its instructions in listing
    order; first in the listing first"""
    index = {b[0]: n for n, b in enumerate(blocks)}
    succ = [[] for _ in blocks]
    for n, (_, ins) in enumerate(blocks):
        falls = True
        for l in ins:
            m = re.match(r"(s_cbranch_\w+|s_branch)\s+(\S+)", l)
            if m and m.group(2) in index:
                succ[n].append(index[m.group(2)])
                falls = falls and m.group(1) != "s_branch"
            if l.startswith("s_endpgm"):
                falls = False
        if falls and n + 1 < len(blocks):
            succ[n].append(n + 1)
    sys.setrecursionlimit(max(10000, sys.getrecursionlimit()))
    order, low, on, stack, comps, count = {}, {}, set(), [], [], [0]

    def visit(v):                                            # Tarjan
        order[v] = low[v] = count[0]
        count[0] += 1
        stack.append(v)
        on.add(v)
        for w in succ[v]:
            if w not in order:
                visit(w)
                low[v] = min(low[v], low[w])
            elif w in on:
                low[v] = min(low[v], order[w])
        if low[v] == order[v]:
            comp = []
            while True:
                w = stack.pop()
                on.discard(w)
                comp.append(w)
                if w == v:
                    break
            if len(comp) > 1 or v in succ[v]:
                comps.append(sorted(comp))
    for v in range(len(blocks)):
        if v not in order:
            visit(v)
    loops = [[l for b in comp for l in blocks[b][1]] for comp in sorted(comps)]
    return [ins for ins in loops if any(l.startswith("global_store") for l in ins)]


def _is_load(l):
    return l.startswith(("global_load", "buffer_load", "flat_load", "scratch_load"))


def _patterns(ins):
    stores = [n for n, l in enumerate(ins) if l.startswith("global_store")]
    between = [l for l in ins[stores[0]:stores[-1] + 1] if _is_load(l)] if stores else []
    return dict(vmcnt0=[l for l in ins if l.startswith("s_waitcnt") and "vmcnt(0)" in l],
                loads_between_stores=between,
                saveexec=sum(l.startswith("s_and_saveexec") for l in ins))


@pytest.mark.parametrize("name", list(KERNELS))
def test_row_loop_patterns(listing, name):
    prefix, nloops, vgpr_before, saveexec = KERNELS[name]
    blocks, fig = _kernel(listing, prefix)
    loops = _store_loops(blocks)
    assert len(loops) == nloops, (name, "loops with global stores", len(loops))
    p = _patterns(loops[0])
    print(name, fig, {k: (v if isinstance(v, int) else len(v)) for k, v in p.items()}, "loop instructions", len(loops[0]))
    assert any(_is_load(l) for l in loops[0]), (name, "the row loop requests the next row")
    assert p["vmcnt0"] == [], (name, "s_waitcnt vmcnt(0) in the row loop")
    assert p["loads_between_stores"] == [], (name, "a load between the row's stores", p["loads_between_stores"])
    assert p["saveexec"] == saveexec, (name, "s_and_saveexec in the row loop", p["saveexec"])
    waits = [int(m) for l in loops[0] if l.startswith("s_waitcnt") for m in re.findall(r"vmcnt\((\d+)\)", l)]
    assert waits and min(waits) >= 3, (name, "every wait leaves at least the three chunks behind it in flight", waits)
    assert fig["spill"] == 0 and fig["lds"] == 0, (name, fig)
    assert fig["vgpr"] <= vgpr_before, (name, "VGPRs", fig["vgpr"], "before", vgpr_before)


def test_layernorm_fwd_patterns(listing):
    prefix, vgpr_before = LN_FWD
    blocks, fig = _kernel(listing, prefix)
    ins = [l for _, b in blocks for l in b]
    p = _patterns(ins)
    print("ln_fwd_kernel<3, full>", fig, {k: (v if isinstance(v, int) else len(v)) for k, v in p.items()}, "instructions", len(ins))
    assert _store_loops(blocks) == [], "one row per wave: no row loop"
    assert p["loads_between_stores"] == []
    # the row (3 loads) and the thread's piece of gamma and of beta (2) are requested together, ahead of the reductions
    loads = [n for n, l in enumerate(ins) if _is_load(l)]
    first_shuffle = min(n for n, l in enumerate(ins) if l.startswith(("ds_bpermute", "ds_swizzle")) or "dpp" in l)
    assert len(loads) == 5 and max(loads) < first_shuffle, (loads, first_shuffle)
    assert len(p["vmcnt0"]) == 1, p["vmcnt0"]               # the row's last chunk, the last load issued: one memory phase
    assert p["saveexec"] == 1, p["saveexec"]                 # lane 0 stores mean / rstd; none guards a chunk
    assert fig["spill"] == 0 and fig["lds"] == 0
    assert fig["vgpr"] <= vgpr_before, (fig["vgpr"], vgpr_before)
