"""The scalar side of an emit tile, read off the gfx950 assembly (no GPU needed: hipcc cross-compiles).

SMEM returns out of order and shares `lgkmcnt` with LDS, so every `s_load` in front of a use costs a full `s_waitcnt lgkmcnt(0)`:
a round trip to the scalar cache that also drains the wave's LDS reads.  The rule of the tile (vg_kernels.hpp, ENTRY_STATE): all
wave-uniform state -- the kernel arguments and, behind their pointer, the camera's intrinsics -- is fetched at entry, and nothing
scalar lies behind the first vector memory access.  For every INLINE_CHAIN frames-in-LDS instantiation of vg_emit_kernel (each
model, with and without Jacobians, each store policy):

1. no `s_load` behind the first `global_load` / `global_store`, except in basic blocks that hold a `global_atomic` (the
   failed-projection CAS block);
2. no `s_load` between the barrier and the residual store, i.e. no `lgkmcnt(0)` there that a scalar load causes;
3. no backward branch that closes a loop behind the residual store outside the CAS block: the chain has one member at compile
   time, the member loop is gone;
4. the headline instantiations (EUCM, Jacobians) hold at most the 96 VGPRs they held before the fetch moved, and no scratch."""
import re

import pytest

from tests import isa
from tests.isa import kernel_metadata
from tests.test_emit_isa_cpu import basic_blocks, kernel_bodies

# vg_emit_kernel<MODEL, WANT_JAC, FRAMES_LDS = true, INLINE_CHAIN = true, POLICY>
INLINE = re.compile(r"^_ZN2vg14vg_emit_kernelILi(\d)ELb([01])ELb1ELb1ELi(\d)EEEvNS_8EmitArgsE$")
HEADLINE = re.compile(r"^_ZN2vg14vg_emit_kernelILi0ELb1ELb1ELb1ELi\dEEEvNS_8EmitArgsE$")
PARENT_HEADLINE_VGPRS = 96
IS_VMEM = ("global_load", "global_store", "buffer_load", "buffer_store", "flat_load", "flat_store")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = isa.hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    return isa.device_asm(hipcc, "vg_emit_tu.hip", str(tmp_path_factory.mktemp("isa_scalar") / "vg_emit_tu.s"))


@pytest.fixture(scope="module")
def inline_kernels(asm):
    out = {k: v for k, v in kernel_bodies(asm).items() if INLINE.match(k)}
    assert {INLINE.match(k).groups() for k in out} == {(m, j, p) for m in "012" for j in "01" for p in "012"}, sorted(out)
    return out


def flat(lines):
    """[(block label, block holds a global atomic, instruction)] in layout order"""
    return [(label, any(x.startswith("global_atomic") for x in ins), x) for label, ins, _ in basic_blocks(lines) for x in ins]


def s_loads_behind_first_vmem(lines):
    seen, bad = False, []
    for label, atomic, x in flat(lines):
        if x.startswith(IS_VMEM):
            seen = True
        elif seen and not atomic and x.startswith(("s_load", "s_buffer_load")):
            bad.append("%s: %s" % (label, x))
    return bad


def barrier_to_residual_store(lines):
    """the instructions from the barrier to the first global store behind it (the residual pair's), in layout order"""
    ins = flat(lines)
    barrier = next(i for i, (_, _, x) in enumerate(ins) if x.startswith("s_barrier"))
    store = next(i for i in range(barrier, len(ins)) if ins[i][2].startswith("global_store"))
    return ins[barrier:store + 1]


def behind_residual_store(lines):
    """what can run once the residual store has been issued: the rest of its block and every block reachable from it (a block the
    compiler laid out behind s_endpgm for a branch of the head is not)"""
    blocks = basic_blocks(lines)
    index = {b[0]: i for i, b in enumerate(blocks)}
    label = barrier_to_residual_store(lines)[-1][0]
    first = index[label]
    ins = blocks[first][1]
    k = next(i for i, x in enumerate(ins) if x.startswith("global_store"))
    atomic = lambda j: any(x.startswith("global_atomic") for x in blocks[j][1])
    out = [(label, atomic(first), x) for x in ins[k + 1:]]
    reached, work = set(), [index[t] for t in blocks[first][2]]
    while work:
        j = work.pop()
        if j not in reached:
            reached.add(j)
            work += [index[t] for t in blocks[j][2]]
    for j in sorted(reached):
        out += [(blocks[j][0], atomic(j), x) for x in blocks[j][1]]
    return out


def loops_behind(lines, behind):
    """the blocks of `behind` (behind_residual_store(lines)) that can reach themselves again -- a loop needs a backward branch, but a
    branch back from a cold block the compiler laid out behind s_endpgm is no loop -- outside blocks with a global atomic"""
    blocks = basic_blocks(lines)
    index = {b[0]: i for i, b in enumerate(blocks)}
    bad = []
    for label in dict.fromkeys(lab for lab, atomic, _ in behind if not atomic):
        reached, work = set(), [index[t] for t in blocks[index[label]][2]]
        while work:
            j = work.pop()
            if j not in reached:
                reached.add(j)
                work += [index[t] for t in blocks[j][2]]
        if index[label] in reached:
            bad.append(label)
    return bad


def test_no_scalar_load_behind_the_first_vector_access(inline_kernels):
    bad = {k: b for k, b in ((k, s_loads_behind_first_vmem(v)) for k, v in inline_kernels.items()) if b}
    assert not bad, bad
    for k, v in inline_kernels.items():   # ... and the state is fetched: the loads are there, in front
        assert any(x.startswith("s_load") for _, _, x in flat(v)), k


def test_no_scalar_load_between_barrier_and_residual_store(inline_kernels):
    for k, v in inline_kernels.items():
        between = barrier_to_residual_store(v)
        assert between[-1][2].startswith("global_store_dwordx4"), (k, between[-1])
        assert not [x for _, atomic, x in between if not atomic and x.startswith(("s_load", "s_buffer_load"))], k


def test_member_loop_is_gone(inline_kernels):
    for k, v in inline_kernels.items():
        behind = behind_residual_store(v)
        assert any(x.startswith("s_endpgm") for _, _, x in behind), k
        assert not loops_behind(v, behind), (k, loops_behind(v, behind))


def test_headline_registers(asm):
    meta = kernel_metadata(asm)
    heads = [k for k in meta if HEADLINE.match(k)]
    assert len(heads) == 3, heads
    for k in heads:
        assert int(meta[k][".vgpr_count"]) + int(meta[k].get(".agpr_count", 0)) <= PARENT_HEADLINE_VGPRS, (k, meta[k][".vgpr_count"])
        assert int(meta[k][".private_segment_fixed_size"]) == 0, k
        assert int(meta[k].get(".vgpr_spill_count", 0)) == 0 and int(meta[k].get(".sgpr_spill_count", 0)) == 0, k


def test_the_analysis_sees_what_it_looks_for():
    """a scalar load behind a vector access counts unless its block holds an atomic; a loop behind the store counts"""
    lines = """
	s_load_dwordx2 s[4:5], s[0:1], 0x0
	s_waitcnt lgkmcnt(0)
	global_load_dwordx4 v[2:5], v[0:1], off
	s_barrier
	s_cbranch_scc1 .LBB0_2
	s_load_dwordx2 s[6:7], s[0:1], 0x60
	global_atomic_cmpswap_x2 v[2:3], v9, v[2:5], s[12:13] sc0
.LBB0_2:
	s_load_dwordx2 s[2:3], s[0:1], 0x20
	global_store_dwordx4 v[0:1], v[2:5], off
.LBB0_3:
	global_store_dwordx4 v[0:1], v[2:5], off
	s_cbranch_scc1 .LBB0_3
	s_endpgm
.LBB0_4:
	s_branch .LBB0_2""".split("\n")
    assert s_loads_behind_first_vmem(lines) == [".LBB0_2: s_load_dwordx2 s[2:3], s[0:1], 0x20"]
    between, behind = barrier_to_residual_store(lines), behind_residual_store(lines)
    assert [x for _, atomic, x in between if not atomic and x.startswith("s_load")] == ["s_load_dwordx2 s[2:3], s[0:1], 0x20"]
    assert loops_behind(lines, behind) == [".LBB0_3"]
