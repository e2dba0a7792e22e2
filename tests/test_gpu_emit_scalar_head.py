"""The one-launch emit tiles fetch their wave-uniform state -- kernel arguments and camera intrinsics -- at entry and hold it in
SGPRs (vg_kernels.hpp: ENTRY_STATE, emit_fetch_args), and their chain has one member at compile time.  Here the cases in which
state that moved can go wrong, at the smallest sizes that reach them: every model (Mei stages its intrinsic rows in half-waves);
3 images x 96 corners (288 observations: the second tile is partial, its last wave half full); a board of 63 corners (a tile
straddles up to 6 images); a board of 3 corners x 200 images (the smallest board whose frames still fit the LDS: up to 87 frames
per tile, the walking lanes span two waves); the NULL-pointer paths (intrinsic block only, member block only, residuals only).

Held to the oracle at the project's bar (tests/parity.py, 1e-10), and byte for byte: one launch against chunked launches of the
same dataset (first_block != 0, offset output pointers), an identity dataset against the same images through a permuted
image_index (seq_index), and the failed-projection count over consecutive evaluations and between chunked and whole."""
import numpy as np
import pytest

from oracle import vgo
from tests.parity import assert_block_parity

pytestmark = pytest.mark.gpu

MODELS = ["eucm", "ucm", "mei"]
SHAPES = [(3, 96), (9, 63), (200, 3)]   # images x corners
MASKS = [None, [True, False], [False, True]]   # every block; jac_intr only; member block only


def _data(model, n_images, n_corners, seed=11):
    from visgeom_amd import synthetic as S

    d = S.make_mono(model, n_images, seed)
    return d["init_intrinsics"], d["init_poses"].copy(), d["board"][:n_corners], np.ascontiguousarray(d["corners"][:, :n_corners])


def _problem(model, intr, poses, board, corners, image_index=None):
    from visgeom_amd import CalibrationProblem

    p = CalibrationProblem(0)
    cam = p.add_camera(model, intr)
    seq = p.add_transform(False, poses)
    ds = p.add_dataset(cam, [(seq, 0)], board, corners, image_index=image_index)
    p.finalize()
    assert p._lib.vg_dataset_single_launch(p._h, ds) == 1
    return p, ds


def _rows(p, ds, want_jac=True, jac_mask=None):
    """one evaluation into NaN-filled arrays -> ([res, jac_intr or None, member block or None] as numpy, failed count)"""
    res, ji, jm = p.alloc_outputs(ds, want_jac=want_jac, jac_mask=jac_mask)
    for t in [res, ji] + list(jm):
        if t is not None:
            t.fill_(float("nan"))
    p.prepare()
    p.evaluate_dataset(ds, res, ji, jm)
    p.synchronize()
    out = [t.cpu().numpy() if t is not None else None for t in [res, ji] + list(jm)]
    for a in out:
        assert a is None or not np.isnan(a).any(), "rows left unwritten"
    return out, p.failed_count(ds)


def _same_bytes(got, ref, what):
    for a, b in zip(got, ref):
        assert (a is None) == (b is None), what
        assert a is None or a.tobytes() == b.tobytes(), what


_ORACLE = {}


def _oracle(model, shape, intr, poses, board, corners):
    """the oracle's rows of a case, computed once"""
    if (model, shape) not in _ORACLE:
        n, K = shape[0], len(intr)
        pv = np.concatenate([np.asarray(intr, float), np.asarray(poses, float).ravel()])
        _ORACLE[model, shape] = vgo.eval_dataset(vgo.MODELS[model], [0], board, corners, pv, 0, [K], [6], np.arange(n), threads=4)
    return _ORACLE[model, shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", MODELS)
def test_rows_equal_the_oracle_with_every_block_and_with_null_blocks(model, shape):
    intr, poses, board, corners = _data(model, *shape)
    r_ref, ji_ref, jm_ref = _oracle(model, shape, intr, poses, board, corners)
    p, ds = _problem(model, intr, poses, board, corners)
    try:
        full = None
        for mask in MASKS:
            (res, ji, jm), failed = _rows(p, ds, jac_mask=mask)
            assert failed == 0
            for b in range(shape[0]):
                assert_block_parity(res[b], [ji[b] if ji is not None else None, jm[b] if jm is not None else None], r_ref[b],
                                    [ji_ref[b] if ji is not None else None, jm_ref[0][b] if jm is not None else None], corners[b],
                                    "%s %s mask %s block %d" % (model, shape, mask, b))
            if mask is None:
                full = (res, ji, jm)
            else:   # a NULL block changes nothing in the blocks that are written
                _same_bytes([res, ji if ji is not None else full[1], jm if jm is not None else full[2]], full, "mask %s" % mask)
        (res, _, _), failed = _rows(p, ds, want_jac=False)   # residuals only: the kernel without Jacobians
        assert failed == 0
        for b in range(shape[0]):
            assert_block_parity(res[b], None, r_ref[b], None, corners[b], "%s %s cost only, block %d" % (model, shape, b))
        assert res.tobytes() == full[0].tobytes()
    finally:
        p.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", MODELS)
def test_chunked_launches_give_the_bytes_of_one_launch(model, shape):
    from visgeom_amd import capi

    n, N = shape
    intr, poses, board, corners = _data(model, *shape)
    p, ds = _problem(model, intr, poses, board, corners)
    per = {3: 2, 9: 4, 200: 199}[n]   # chunks of whole images, the last one a single image
    assert n % per == 1
    try:
        for want_jac, mask in [(True, None), (True, [False, True]), (False, None)]:
            capi.debug_set("max_obs_per_launch", 0)
            whole, f0 = _rows(p, ds, want_jac, mask)
            capi.debug_set("max_obs_per_launch", per * N)
            chunked, f1 = _rows(p, ds, want_jac, mask)
            _same_bytes(chunked, whole, "%s %s chunks of %d images" % (model, shape, per))
            assert f0 == f1 == 0
    finally:
        capi.debug_set("max_obs_per_launch", 0)
        p.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", MODELS)
def test_permuted_image_index_gives_the_bytes_of_the_identity_dataset(model, shape):
    n = shape[0]
    intr, poses, board, corners = _data(model, *shape)
    perm = np.random.default_rng(5).permutation(n).astype(np.int32)
    assert not np.array_equal(perm, np.arange(n))
    poses_perm = np.empty_like(poses)
    poses_perm[perm] = poses   # image b of the dataset reads element perm[b] of the sequence: its own pose
    p, ds = _problem(model, intr, poses, board, corners)
    q, dq = _problem(model, intr, poses_perm, board, corners, image_index=perm)
    try:
        ref, f0 = _rows(p, ds)
        got, f1 = _rows(q, dq)
        _same_bytes(got, ref, "%s %s" % (model, shape))
        assert f0 == f1 == 0
    finally:
        p.close()
        q.close()


def _behind_problem(model):
    intr, poses, board, corners = _data(model, 6, 96)   # 576 observations: tiles of images 0-2, 2-5, 5
    poses[0] = [0, 0, -1, 0, 0, 0]   # the board behind the camera: tile 0
    poses[5] = [0, 0, -1, 0, 0, 0]   # tiles 1 and 2; alone in the second launch when chunked
    return _problem(model, intr, poses, board, corners)


@pytest.mark.parametrize("model", ["eucm"])   # the model whose projection fails for a board behind the camera at these intrinsics
def test_failed_count_is_the_same_on_consecutive_evaluations(model):
    p, ds = _behind_problem(model)
    try:
        counts = [_rows(p, ds)[1] for _ in range(3)]
        assert counts[0] >= 2 and counts == [counts[0]] * 3, counts
        res = _rows(p, ds)[0][0]
        assert int((res == 1e15).sum()) == 2 * counts[0]   # the in-band failure value, a pair per failed corner
    finally:
        p.close()


@pytest.mark.parametrize("model", ["eucm"])   # the model whose projection fails for a board behind the camera at these intrinsics
def test_failed_count_chunked_equals_whole(model):
    from visgeom_amd import capi

    p, ds = _behind_problem(model)
    try:
        whole, f0 = _rows(p, ds)
        capi.debug_set("max_obs_per_launch", 5 * 96)   # images 0-4, then image 5 alone
        chunked, f1 = _rows(p, ds)
        assert f0 == f1 >= 2
        _same_bytes(chunked, whole, model)
    finally:
        capi.debug_set("max_obs_per_launch", 0)
        p.close()
