"""The head of an emit tile, read off the gfx950 assembly (no GPU needed: hipcc cross-compiles).

A workgroup has nothing in flight until its first store.  The headline instantiation (EUCM, Jacobians, frames in LDS, the
chain walked in the kernel) therefore sends the residual pair off BEFORE the Jacobian arithmetic: in program order the residual
`global_store_dwordx4` precedes the first `ds_write` of a Jacobian row block, and the FP64 divisions that only the Jacobians need
(eucm.h: 1 / eta / eta, alpha beta / rho, alpha z / rho, two per intrinsic row pair) come behind it.  In front of it stay the
projection's own: x / eta, y / eta and the two of the hemisphere test; those of the walk lie in front of the barrier.  The chain-parameter load is the
first global load of the kernel, ahead of the board and observation loads."""
import re

import pytest

from tests import isa

HEADLINE = re.compile(r"^_ZN2vg14vg_emit_kernelILi0ELb1ELb1ELb1ELi(\d)EEEvNS_8EmitArgsE$")  # EUCM, Jacobians, frames in LDS, inline chain


@pytest.fixture(scope="module")
def heads(tmp_path_factory):
    hipcc = isa.hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    text = isa.device_asm(hipcc, "vg_emit_tu.hip", str(tmp_path_factory.mktemp("isa_head") / "vg_emit_tu.s"))
    out = {}
    for m in re.finditer(r"^(_Z\w+):", text, flags=re.M):
        if HEADLINE.match(m.group(1)):
            body = text[m.end():text.find(".Lfunc_end", m.end())]
            out[m.group(1)] = [ln.split(";")[0].strip() for ln in body.split("\n")]
    assert len(out) == 3, sorted(out)   # one per store policy
    return out


def _first(lines, prefix, start=0):
    for i in range(start, len(lines)):
        if lines[i].startswith(prefix):
            return i
    return None


def test_residual_store_precedes_the_jacobian_row_blocks(heads):
    for name, lines in heads.items():
        store = _first(lines, "global_store_dwordx4")
        assert store is not None, name
        row_write = _first(lines, "ds_write", store)
        assert row_write is not None, name
        # no staging write of a row block in front of the residual store (the walk's frame writes are ds_write_b64 / b128 of the
        # <= 4 walking lanes, in front of the barrier; the row blocks' are behind it)
        barrier = _first(lines, "s_barrier")
        assert barrier is not None and barrier < store, name
        assert _first(lines[:store], "ds_write", barrier) is None, (name, "a row block is staged before the residual pair leaves")


def test_jacobian_divisions_follow_the_residual_store(heads):
    for name, lines in heads.items():
        store = _first(lines, "global_store_dwordx4")
        barrier = _first(lines, "s_barrier")
        between = sum(1 for x in lines[barrier:store] if x.startswith("v_div_fmas_f64"))
        behind = sum(1 for x in lines[store:] if x.startswith("v_div_fmas_f64"))
        assert between <= 4, (name, between)   # x / eta, y / eta; z / eta and the bound C of the hemisphere test
        assert behind >= 5, (name, behind)     # the Jacobians' own divisions
        # ... and nothing of the projection a second time: the Jacobians have ten divisions (six of the intrinsic rows, four of the
        # projection Jacobian) and share rho and eta with the projection, so no square root follows the store
        assert behind <= 10, (name, behind)
        assert not [x for x in lines[store:] if x.startswith(("v_sqrt_f64", "v_rsq_f64"))], name


def test_merged_emit_kernel_keeps_four_waves_and_no_scratch(tmp_path):
    """vg_emit_multi_kernel (stereo, rig), every store policy: <= 128 VGPRs (four waves per SIMD) and no scratch"""
    hipcc = isa.hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    meta = isa.kernel_metadata(isa.device_asm(hipcc, "vg_emit_tu.hip", str(tmp_path / "vg_emit_tu.s")))
    multi = [k for k in meta if "vg_emit_multi_kernel" in k]
    assert len(multi) == 3, multi
    for k in multi:
        assert int(meta[k][".vgpr_count"]) + int(meta[k].get(".agpr_count", 0)) <= 128, (k, meta[k][".vgpr_count"])
        assert int(meta[k][".private_segment_fixed_size"]) == 0, k


def test_chain_parameters_are_the_first_load(heads):
    for name, lines in heads.items():
        # the optional seq_index word (a 4-byte load on its own branch, NULL for an identity index) belongs to the same chain
        loads = [x for x in lines if x.startswith("global_load") and not x.startswith("global_load_dword ")]
        assert loads, name
        # the six doubles of the walking lane's pose: 16-byte loads; the board is read in 8-byte pieces (3 doubles per corner)
        assert loads[0].startswith("global_load_dwordx4"), (name, loads[:4])
        first_load = _first(lines, "global_load")
        # the per-lane division by N (v_rcp_iflag_f32 of the unsigned division expansion) has not started yet: at most the
        # wave-uniform one of the tile's first image in front of the load
        assert sum(1 for x in lines[:first_load] if x.startswith("v_rcp_iflag_f32")) <= 2, name
