"""The store policy of MERGED emit launches (vg_problem_evaluate -> vg_emit_multi_kernel: stereo pair, camera rig) inside the
Infinity Cache: plain write-back stores or write-through (`sc1`) stores, switched by the hook emit_write_through (-1 = plain,
0 = the library's choice: write-through up to 230 MB per launch).  The policy changes where the lines wait, never what is written: every row of
every dataset and every failed-projection count must be the same BIT FOR BIT."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rows(p, dss):
    outs = [p.alloc_outputs(ds) for ds, _, _, _ in dss]
    for res, ji, jm in outs:
        for t in [res, ji] + list(jm):
            t.fill_(float("nan"))
    p.prepare()
    p.evaluate_all(outs)
    p.synchronize()
    rows = []
    for res, ji, jm in outs:
        rows += [res.cpu().numpy(), ji.cpu().numpy()] + [m.cpu().numpy() for m in jm]
    return rows, [p.failed_count(ds) for ds, _, _, _ in dss]


@pytest.mark.parametrize("cfg,images", [
    (3, 37),     # stereo: 2 x 3 552 observations, 13.9 tiles per dataset: partial last tiles
    (3, 600),
    (5, 211),    # rig [UCM, EUCM, EUCM, Mei]: the model switch and Mei's half-wave staging in one launch
    (5, 1000),
])
def test_merged_write_through_rows_equal_the_plain_rows(cfg, images):
    from visgeom_amd import benchlib, capi

    p, dss, _, _ = benchlib.build(cfg, images=images)
    try:
        capi.debug_set("emit_write_through", -1)
        ref, ref_failed = _rows(p, dss)
        for a in ref:
            assert not np.isnan(a).any()
        for k in (0,):
            capi.debug_set("emit_write_through", k)
            got, failed = _rows(p, dss)
            assert failed == ref_failed, k
            for a, b in zip(got, ref):
                assert a.tobytes() == b.tobytes(), "store policy %d changes the rows of a merged launch" % k
    finally:
        capi.debug_set("emit_write_through", 0)
        p.close()
