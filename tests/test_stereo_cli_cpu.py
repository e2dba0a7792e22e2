"""The stereo front ends without a GPU: visgeom_amd.stereo.params_from_json reads the reference's ex_epipolar_stereo.json the
way SgmParameters does, and the `stereo` program rejects malformed input with one line on stderr before any GPU work."""
import copy
import json
import os
import subprocess

import numpy as np
import pytest

from tests import stereo_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "tests", "golden", "ex_epipolar_stereo.json")


def test_params_from_json_reads_the_reference_example():
    from visgeom_amd import stereo

    sp = json.load(open(EXAMPLE))["stereo_parameters"]
    p = stereo.params_from_json(sp)
    assert (p.scale, p.u0, p.v0, p.u_max, p.v_max) == (1, 50, 50, 1280, 800)
    assert p.equal_margins == 1
    assert (p.x_max, p.y_max) == (1, 1)   # "xMax_" / "yMax_" are not keys; equal_margins sets the size at creation
    assert (p.disp_max, p.error_max, p.verbosity, p.hypotheses, p.hypo_difference, p.flaw_cost, p.desc_length,
            p.desc_resp_thresh) == (120, 150, 1, 1, 10, 25, 15, 2)
    assert list(p.scales)[:p.n_scales] == [1, 2, 3, 5] and p.n_scales == 4
    assert (p.step_cost, p.jump_cost, p.image_based_cost, p.salient_points_only, p.use_uv_cache) == (5, 32, 1, 1, 0)
    assert p.epipole_margin == 2500 and p.num_epipolar_planes == 2000


def test_params_from_json_key_placement():
    from visgeom_amd import stereo

    sp = {"num_epipolar_planes": 64, "epipole_margin": 9, "disparity_max": 8, "use_uv_cache": False,
          "stereo_parameters": {"epipole_margin": 12, "scales_": [7]},
          "sgm_stereo_parameters": {"image_based_cost": False, "salient_points_only": 0, "use_uv_cache": 1, "jump_cost": 40}}
    p = stereo.params_from_json(sp)
    # the reference reads num_epipolar_planes / epipole_margin / disparity_max only inside "stereo_parameters"
    assert p.num_epipolar_planes == 2000 and p.disp_max == 48
    assert p.epipole_margin == 144   # squared
    assert list(p.scales)[:p.n_scales] == [1, 2, 3, 5]
    assert (p.image_based_cost, p.salient_points_only, p.use_uv_cache, p.jump_cost) == (0, 0, 1, 40)
    p = stereo.params_from_json({"stereo_parameters": {"num_epipolar_planes": 64}, "equal_margins": False})
    assert p.num_epipolar_planes == 64 and p.equal_margins == 0


@pytest.fixture(scope="module")
def cli():
    from visgeom_amd import _build

    _build.build()
    return _build.STEREO_CLI


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (93, 125), dtype=np.uint8)
    return img, img, None, stereo_scene.RIGS["sideways"]


def _run(cli, path):
    return subprocess.run([cli, path], capture_output=True, text=True, timeout=60)


def _rejected(r, *words):
    assert r.returncode == 1, (r.returncode, r.stderr)
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("stereo: "), r.stderr
    for w in words:
        assert w in lines[0], lines[0]


def test_cli_usage(cli):
    r = subprocess.run([cli], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage: stereo file.json" in r.stderr


def test_cli_rejects_malformed_json(cli, tmp_path):
    path = tmp_path / "bad.json"
    path.write_text('{"camera_params_left": [1, 2, ')
    _rejected(_run(cli, str(path)), "bad.json")
    path.write_text('{"camera_params_left": [0.6, 1, 60, 60, 62, 46]}')
    _rejected(_run(cli, str(path)), "camera_params_right")


def test_cli_rejects_missing_and_non_p5_images(cli, tmp_path, images):
    path = stereo_scene.write_case(str(tmp_path), "sideways", stereo_scene.SCENE_JSON_PARAMS, images)
    os.remove(tmp_path / "right.pgm")
    _rejected(_run(cli, path), "right.pgm")
    (tmp_path / "right.pgm").write_bytes(b"P2\n125 93\n255\n" + b"0 " * (125 * 93))
    _rejected(_run(cli, path), "not a binary PGM")
    (tmp_path / "right.pgm").write_bytes(b"P5\n125 93\n255\n" + b"\0" * 100)
    _rejected(_run(cli, path), "truncated")


def test_cli_rejects_wrong_image_size(cli, tmp_path, images):
    path = stereo_scene.write_case(str(tmp_path), "sideways", stereo_scene.SCENE_JSON_PARAMS, images)
    stereo_scene.write_pgm(str(tmp_path / "left.pgm"), np.zeros((93, 124), np.uint8))
    _rejected(_run(cli, path), "124 x 93", "125 x 93")


def test_cli_rejects_hypotheses_2(cli, tmp_path, images):
    sp = copy.deepcopy(stereo_scene.SCENE_JSON_PARAMS)
    sp["stereo_parameters"]["hypotheses"] = 2
    path = stereo_scene.write_case(str(tmp_path), "sideways", sp, images)
    _rejected(_run(cli, path), "hypotheses")
    assert not (tmp_path / "depth.pfm").exists()
