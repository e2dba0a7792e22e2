"""The emit kernels' store path, read off the gfx950 assembly (no GPU needed: hipcc cross-compiles).

The emit kernel is store bound.  On CDNA `vmcnt` counts stores as well as loads, so an `s_waitcnt vmcnt` after a tile's
first global store holds the wave until its own stores are acknowledged, with no new bytes in flight.  Every frames-in-LDS
instantiation of vg_emit_kernel (each model, with and without Jacobians, each store policy) must therefore run no vmcnt
wait from its first store to s_endpgm, outside the failed-projection CAS block (the only block with a global atomic).
The headline instantiation must also keep 4 waves per SIMD (<= 128 VGPRs) and use no scratch."""
import re

import pytest

from tests import isa
from tests.isa import kernel_metadata

# vg_emit_kernel<MODEL, WANT_JAC, FRAMES_LDS = true, INLINE_CHAIN[, POLICY]>
EMIT_LDS = re.compile(r"^_ZN2vg14vg_emit_kernelILi(\d)ELb([01])ELb1ELb([01])(?:ELi(\d))?EEEvNS_8EmitArgsE$")
HEADLINE = re.compile(r"^_ZN2vg14vg_emit_kernelILi0ELb1ELb1ELb1E")  # EUCM, Jacobians, frames in LDS, inline chain


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = isa.hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    return isa.device_asm(hipcc, "vg_emit_tu.hip", str(tmp_path_factory.mktemp("isa") / "vg_emit_tu.s"))


def kernel_bodies(text):
    """kernel name -> its instruction lines (from its label to .Lfunc_end)"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):", text, flags=re.M):
        end = text.find(".Lfunc_end", m.end())
        out[m.group(1)] = text[m.end():end].split("\n")
    return out


def basic_blocks(lines):
    """[(label, instructions, successor labels)] in layout order"""
    raw = [["<entry>", []]]
    for ln in lines:
        s = ln.split(";")[0].strip()
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            raw.append([m.group(1), []])
        elif s and not s.startswith("."):
            raw[-1][1].append(s)
    blocks = []
    for i, (label, ins) in enumerate(raw):
        succ = [m.group(2) for x in ins for m in [re.match(r"^s_(cbranch_\w+|branch)\s+(\.LBB\w+)", x)] if m]
        last = ins[-1] if ins else ""
        if not last.startswith(("s_branch", "s_endpgm", "s_setpc")) and i + 1 < len(raw):
            succ.append(raw[i + 1][0])
        blocks.append((label, ins, succ))
    return blocks


def vmcnt_waits_after_store(lines):
    """s_waitcnt instructions with a vmcnt that can run once a global store has been issued (any control-flow path),
    outside the blocks that hold a global atomic"""
    blocks = basic_blocks(lines)
    index = {b[0]: i for i, b in enumerate(blocks)}
    is_vmem_write = lambda x: x.startswith(("global_store", "buffer_store", "flat_store"))
    reached, work = set(), []
    for _, ins, succ in blocks:
        if any(is_vmem_write(x) for x in ins):
            work += [index[s] for s in succ]
    while work:
        j = work.pop()
        if j not in reached:
            reached.add(j)
            work += [index[s] for s in blocks[j][2]]
    waits = []
    for i, (label, ins, _) in enumerate(blocks):
        if any(x.startswith("global_atomic") for x in ins):
            continue
        seen = i in reached
        for x in ins:
            if is_vmem_write(x):
                seen = True
            elif seen and x.startswith("s_waitcnt") and "vmcnt" in x:
                waits.append("%s: %s" % (label, x))
    return waits


def test_frames_in_lds_emit_kernels_never_wait_on_their_stores(asm):
    bodies = kernel_bodies(asm)
    lds = {k: v for k, v in bodies.items() if EMIT_LDS.match(k)}
    # every model with and without Jacobians, walking the chain itself or reading prepared frames
    assert {(EMIT_LDS.match(k).group(1), EMIT_LDS.match(k).group(2), EMIT_LDS.match(k).group(3)) for k in lds} == \
        {(m, j, i) for m in "012" for j in "01" for i in "01"}
    bad = {}
    for name, lines in lds.items():
        assert any(x.strip().startswith("global_store") for x in lines), name
        waits = vmcnt_waits_after_store(lines)
        if waits:
            bad[name] = waits
    assert not bad, bad


def test_headline_emit_kernel_keeps_four_waves_and_no_scratch(asm):
    meta = kernel_metadata(asm)
    heads = [k for k in meta if HEADLINE.match(k)]
    assert heads
    for k in heads:
        assert int(meta[k][".vgpr_count"]) + int(meta[k].get(".agpr_count", 0)) <= 128, (k, meta[k][".vgpr_count"])
        assert int(meta[k][".private_segment_fixed_size"]) == 0, k
        assert int(meta[k].get(".vgpr_spill_count", 0)) == 0, k


def test_wait_counter_sees_a_wait_behind_a_store():
    """the analysis itself: a wait on a path after a store counts, one before the store or in an atomic block does not"""
    lines = """
	global_load_dwordx4 v[2:5], v[0:1], off
	s_waitcnt vmcnt(0)
	s_cbranch_execz .LBB0_2
	global_store_dwordx4 v[0:1], v[2:5], off
.LBB0_2:
	s_cbranch_scc1 .LBB0_4
	global_atomic_cmpswap_x2 v[2:3], v9, v[2:5], s[12:13] sc0
	s_waitcnt vmcnt(0)
.LBB0_4:
	s_waitcnt vmcnt(0) lgkmcnt(0)
	s_endpgm""".split("\n")
    assert vmcnt_waits_after_store(lines) == [".LBB0_4: s_waitcnt vmcnt(0) lgkmcnt(0)"]
