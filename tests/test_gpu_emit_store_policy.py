"""The store policy of the emit launches inside the Infinity Cache (vg_kernels.hpp: stream_store16, vg_emit_launch.hpp: emit_store_policy):
write-through (`sc1`) 16-byte stores by default, plain write-back stores under the hook emit_write_through = -1.  The policy changes
where the lines wait, never what is written: both must give the same rows BIT FOR BIT, the failed-projection count included."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _problem(model, n_images, seed, n_corners=96, behind=()):
    from visgeom_amd import CalibrationProblem, synthetic as S

    d = S.make_mono(model, n_images, seed)
    poses = d["init_poses"].copy()
    for i in behind:   # the board behind the camera: most of that image's corners fail to project
        poses[i] = [0, 0, -1, 0, 0, 0]
    p = CalibrationProblem(0)
    cam = p.add_camera(model, d["init_intrinsics"])
    seq = p.add_transform(False, poses)
    ds = p.add_dataset(cam, [(seq, 0)], d["board"][:n_corners], np.ascontiguousarray(d["corners"][:, :n_corners]))
    p.finalize()
    assert p._lib.vg_dataset_single_launch(p._h, ds) == 1
    return p, ds


def _rows(p, ds, want_jac=True):
    res, ji, jm = p.alloc_outputs(ds, want_jac=want_jac)
    for t in [res, ji] + list(jm or []):
        if t is not None:
            t.fill_(float("nan"))
    p.prepare()
    if want_jac:
        p.evaluate_dataset(ds, res, ji, jm)
    else:
        p.evaluate_dataset(ds, res)
    p.synchronize()
    out = [res.cpu().numpy()]
    if want_jac:
        out += [ji.cpu().numpy()] + [m.cpu().numpy() for m in jm]
    return out, p.failed_count(ds)


def _same(p, ds, forms=(0,), want_jac=True):
    from visgeom_amd import capi

    try:
        capi.debug_set("emit_write_through", -1)
        ref, ref_failed = _rows(p, ds, want_jac)
        for a in ref:
            assert not np.isnan(a).any()
        for k in forms:
            capi.debug_set("emit_write_through", k)
            got, failed = _rows(p, ds, want_jac)
            assert failed == ref_failed, k
            for a, b in zip(got, ref):
                assert a.tobytes() == b.tobytes(), "write-through stores change the rows"
    finally:
        capi.debug_set("emit_write_through", 0)
    return ref_failed


@pytest.mark.parametrize("model,n_images,n_corners", [
    ("eucm", 2, 96),       # one partial tile
    ("eucm", 43, 96),      # 4 128 observations: 17 tiles, the last one partial
    ("ucm", 301, 96),
    ("mei", 683, 96),      # 257 tiles
    ("eucm", 517, 63),     # a board of 63 corners (does not divide 256): a tile touches up to 6 images
    ("mei", 97, 63),
])
def test_write_through_rows_equal_the_plain_rows(model, n_images, n_corners):
    p, ds = _problem(model, n_images, 7, n_corners)
    try:
        _same(p, ds)
    finally:
        p.close()


def test_headline_size():
    p, ds = _problem("eucm", 10000, 3)   # the bench.py step: 199.7 MB of output, inside the cache
    try:
        _same(p, ds)
    finally:
        p.close()


def test_cost_only():
    p, ds = _problem("mei", 683, 5)
    try:
        _same(p, ds, want_jac=False)
    finally:
        p.close()


def test_failures_over_several_tiles_counted_exactly_over_consecutive_epochs():
    # failing images spread over many tiles
    behind = [3, 40, 300, 2700, 2701, 5990]
    p, ds = _problem("eucm", 6000, 4, behind=behind)
    from visgeom_amd import capi

    try:
        failed = _same(p, ds)
        assert failed >= len(behind)   # at least one failing corner in each of those images
        capi.debug_set("emit_write_through", 0)
        for _ in range(3):   # every evaluation is a new epoch: the count restarts, it does not accumulate
            _, n = _rows(p, ds)
            assert n == failed
    finally:
        capi.debug_set("emit_write_through", 0)
        p.close()


def test_chunked_launches():
    from visgeom_amd import capi

    p, ds = _problem("ucm", 1000, 6)
    try:
        capi.debug_set("max_obs_per_launch", 96 * 333)   # four launches, the last one of one image
        _same(p, ds)
    finally:
        capi.debug_set("max_obs_per_launch", 0)
        p.close()
