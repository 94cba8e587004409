"""Lifetime of the side-library handles and of the user-facing classes over them, on device 0.  No kernel is launched."""
import pytest

from tomography_alignment_amd import _fbp_lib, _fsc_lib, _lib, _phase_lib, _prep_lib, _pyr_lib, _xcorr_lib, multires, preprocess, resolution

pytestmark = pytest.mark.gpu

HANDLES = [_xcorr_lib.XcorrHandle, _fbp_lib.FbpHandle, _prep_lib.PrepHandle, _pyr_lib.PyrHandle, _fsc_lib.FscHandle, _phase_lib.PhaseHandle]
OWNERS = [(preprocess.Preprocessor, _prep_lib.PrepHandle), (multires.Pyramid, _pyr_lib.PyrHandle), (resolution.Resolution, _fsc_lib.FscHandle)]


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


@pytest.mark.parametrize("cls", HANDLES[1:], ids=[c.NAME for c in HANDLES[1:]])
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
