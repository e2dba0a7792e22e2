"""visgeom_amd/_handle.py without a GPU and without the library: the life of a handle against a stub destroy function, and the
argument checks the wrappers share."""
import ctypes

import numpy as np
import pytest

from visgeom_amd import _handle, capi, stereo


class Stub:
    def __init__(self):
        self.destroyed = []

    def vg_stub_destroy(self, h):
        self.destroyed.append(h.value)


class Thing(_handle.Handle):
    _destroy = "vg_stub_destroy"

    def __init__(self, value=None):
        if value is None:
            raise ValueError("refused before the handle exists")
        self._h = ctypes.c_void_p(value)


@pytest.fixture
def lib(monkeypatch):
    stub = Stub()
    monkeypatch.setattr(capi, "load", lambda: stub)
    return stub


def test_close_twice_destroys_once(lib):
    t = Thing(0x1234)
    t.close()
    assert lib.destroyed == [0x1234] and t._h is None
    t.close()
    del t
    assert lib.destroyed == [0x1234]


def test_del_closes_an_open_handle_and_leaves_a_null_one_alone(lib):
    t = Thing(0x77)
    del t
    assert lib.destroyed == [0x77]
    t = Thing(0)   # create failed inside the library: the handle stayed NULL
    t.close()
    assert lib.destroyed == [0x77]


def test_del_of_an_object_whose_init_raised_does_nothing(lib):
    t = Thing.__new__(Thing)
    with pytest.raises(ValueError):
        t.__init__()
    assert not hasattr(t, "_h")
    t.__del__()
    t.close()
    assert lib.destroyed == []


def test_a_destroy_that_raises_does_not_escape_del_and_is_not_repeated(monkeypatch):
    calls = []

    class Bad:
        def vg_stub_destroy(self, h):
            calls.append(h.value)
            raise RuntimeError("the library is gone")

    monkeypatch.setattr(capi, "load", lambda: Bad())
    t = Thing(5)
    t.__del__()
    t.__del__()
    assert calls == [5]


def test_every_wrapper_names_its_destroy_function_and_keeps_none_of_its_own():
    from visgeom_amd import depth_fusion, mapping, mono_odom, motion_stereo, photometric, sparse_odom

    names = {stereo.Stereo: "vg_stereo_destroy", motion_stereo.MotionStereo: "vg_motion_stereo_destroy",
             depth_fusion.DepthFusion: "vg_depth_fusion_destroy", photometric.Photometric: "vg_photometric_destroy",
             sparse_odom.SparseOdometry: "vg_sparse_odom_destroy", mono_odom.MonoOdometry: "vg_mono_odom_destroy",
             mapping.PhotometricMapping: "vg_mapping_destroy"}
    for cls, name in names.items():
        assert issubclass(cls, _handle.Handle) and cls._destroy == name
        for method in ("close", "__del__", "_open", "_enter", "_leave"):
            assert method not in vars(cls), (cls.__name__, method)
    # the two frame loops keep none of what their base holds either
    for cls in (mono_odom.MonoOdometry, mapping.PhotometricMapping):
        assert issubclass(cls, _handle.LoopHandle) and cls._destroy == cls._prefix + "destroy"
        for method in ("__init__", "_image", "_depth", "_feed_image", "_get6", "_geti", "map"):
            assert method not in vars(cls) and method not in vars(_handle.Handle), (cls.__name__, method)


def test_vec():
    v = _handle._vec([1, 2, 3, 4, 5, 6], 6, "xi")
    assert v.dtype == np.float64 and v.flags.c_contiguous and v.tolist() == [1., 2., 3., 4., 5., 6.]
    assert _handle._vec(np.arange(6).reshape(2, 3), 6, "xi").shape == (6,)
    for bad in ([1, 2, 3, 4, 5], np.zeros(7), []):
        with pytest.raises(ValueError, match="xi must have 6 values"):
            _handle._vec(bad, 6, "xi")
    assert stereo._vec is _handle._vec   # the name other modules and tests take it by


def test_u8_images_refuses_what_is_not_a_uint8_cuda_image_of_the_size():
    torch = pytest.importorskip("torch")
    text = r"img must be a uint8 CUDA tensor \[n, 4, 6\] or \[4, 6\]"
    for bad in (torch.zeros((4, 6), dtype=torch.uint8),                  # a CPU tensor
                torch.zeros((4, 6), dtype=torch.uint8, device="meta"),   # not CUDA
                torch.zeros((4, 6), dtype=torch.float32),                # wrong dtype
                torch.zeros((6, 4), dtype=torch.uint8),                  # wrong trailing shape
                np.zeros((4, 6), np.uint8), None):
        with pytest.raises(ValueError, match=text) as e:
            _handle._u8_images(bad, 4, 6, "img")
        assert "CUDA" in str(e.value)


def test_f64_cuda_refuses_what_is_not_a_float64_cuda_tensor_of_the_shape():
    torch = pytest.importorskip("torch")
    for bad in (torch.zeros((5, 3), dtype=torch.float64),                  # a CPU tensor
                torch.zeros((5, 3), dtype=torch.float64, device="meta"),   # not CUDA
                torch.zeros((5, 3), dtype=torch.float32),                  # wrong dtype
                torch.zeros((5, 2), dtype=torch.float64),                  # wrong trailing shape
                np.zeros((5, 3)), None):
        with pytest.raises(ValueError, match=r"x1 must be a float64 CUDA tensor \[n, 3\]"):
            _handle._f64_cuda(bad, (3,), "x1")
    with pytest.raises(ValueError, match=r"size must be a float64 CUDA tensor \[n\]$"):
        _handle._f64_cuda(torch.zeros((5, 1), dtype=torch.float64), (), "size")
