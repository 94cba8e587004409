"""Lifetime of every side-library handle and of every user-facing class over one, on device 0.  No kernel is launched."""
import pytest

import abi

from tomography_alignment_amd import (_cor_lib, _fsc_lib, _half_lib, _lib, _mesh_lib, _mom_lib, _morph_lib, _phase_lib, _prep_lib, _pyr_lib,
                                      _seg_lib, _vol_lib, _vreg_lib, half_acquisition, mesh, morphology, multires, postprocess, preprocess,
                                      registration, resolution, rotation_axis, segment)
from tomography_alignment_amd.align import consistency

pytestmark = pytest.mark.gpu

HANDLES = [lib.handle for lib in abi.libraries() if lib.handle is not None]
# XcorrHandle takes its device modulo the device count, as _lib.Context does, so none is out of range for it; tomo_xcorr_create itself
# refuses one in the same words as the others
RANGE_CHECKED = [cls for cls in HANDLES if cls.NAME != "xcorr"]
# every _ops.HandleOwner and the handle it makes
OWNERS = [(preprocess.Preprocessor, _prep_lib.PrepHandle), (multires.Pyramid, _pyr_lib.PyrHandle), (resolution.Resolution, _fsc_lib.FscHandle),
          (registration.Registrar, _vreg_lib.VregHandle), (consistency.Consistency, _mom_lib.MomHandle),
          (rotation_axis.RotationAxis, _cor_lib.CorHandle), (half_acquisition.HalfAcquisition, _half_lib.HalfHandle),
          (postprocess.PostProcessor, _vol_lib.VolHandle), (segment.Segmenter, _seg_lib.SegHandle),
          (morphology.Morphology, _morph_lib.MorphHandle), (mesh.MeshExtractor, _mesh_lib.MeshHandle)]


def test_the_lists_are_whole():
    from tomography_alignment_amd import _ops
    assert len(HANDLES) == 15
    found, todo = set(), [_ops.HandleOwner]
    while todo:
        for sub in todo.pop().__subclasses__():
            if sub.__module__.startswith("tomography_alignment_amd."):
                found.add(sub)
                todo.append(sub)
    assert found == set(cls for cls, _ in OWNERS) and len(OWNERS) == 11


@pytest.mark.parametrize("cls", HANDLES, ids=[c.NAME for c in HANDLES])
def test_close_is_idempotent_and_final(cls):
    h = cls(0)
    assert h.handle and h.device == 0
    h.close()
    h.close()
    with pytest.raises(_lib.TomoError, match="^%s handle closed$" % cls.NAME):
        h.handle
    with cls(0) as h2:
        assert h2.handle
    with pytest.raises(_lib.TomoError, match="^%s handle closed$" % cls.NAME):
        h2.handle


@pytest.mark.parametrize("cls", RANGE_CHECKED, ids=[c.NAME for c in RANGE_CHECKED])
def test_a_device_out_of_range_is_refused(cls):
    with pytest.raises(_lib.TomoError, match="device out of range"):
        cls(10**6)


@pytest.mark.parametrize("cls,handle_cls", OWNERS, ids=[c.__name__ for c, _ in OWNERS])
def test_a_context_of_its_own_is_closed_with_it(cls, handle_cls):
    live = len(_lib.LIVE_CONTEXTS)
    p = cls()
    p._ready(None)
    ctx, h = p.ctx, p.handle
    assert isinstance(h, handle_cls) and h.handle and ctx.handle and len(_lib.LIVE_CONTEXTS) == live + 1
    p.close()
    assert p.ctx is None and p.handle is None and len(_lib.LIVE_CONTEXTS) == live
    with pytest.raises(_lib.TomoError, match="handle closed"):
        h.handle
    with pytest.raises(_lib.TomoError, match="context closed"):
        ctx.handle
    p.close()


@pytest.mark.parametrize("cls,handle_cls", OWNERS, ids=[c.__name__ for c, _ in OWNERS])
def test_a_given_context_stays_open(cls, handle_cls):
    ctx = _lib.Context(0)
    live = len(_lib.LIVE_CONTEXTS)
    with cls(ctx) as p:
        p._ready(None)
        h = p.handle
        assert p.ctx is ctx and h.device == ctx.device and len(_lib.LIVE_CONTEXTS) == live
    assert p.handle is None and p.ctx is ctx and ctx.handle and len(_lib.LIVE_CONTEXTS) == live
    with pytest.raises(_lib.TomoError, match="handle closed"):
        h.handle
    ctx.close()


def test_the_preprocessor_closes_its_phase_handle_too():
    live = len(_lib.LIVE_CONTEXTS)
    p = preprocess.Preprocessor()
    p._ready_phase(None)
    ph = p._phase
    assert isinstance(ph, _phase_lib.PhaseHandle) and ph.handle and p.handle is None and len(_lib.LIVE_CONTEXTS) == live + 1
    p.close()
    assert p._phase is None and p.ctx is None and len(_lib.LIVE_CONTEXTS) == live
    with pytest.raises(_lib.TomoError, match="^phase handle closed$"):
        ph.handle
