"""The shared binding layer (tomography_alignment_amd/_binding.py) as the seven binding modules use it: needs the built libraries, no GPU."""
import ctypes

import pytest

from tomography_alignment_amd import _binding, _fbp_lib, _fsc_lib, _lib, _phase_lib, _prep_lib, _pyr_lib, _xcorr_lib

# module, library name (libtomo_<name>.so), symbol prefix, directory of its Makefile
MODULES = [
    (_lib, "hip", "tomo_", "tomography_alignment_amd/csrc"),
    (_xcorr_lib, "xcorr", "tomo_xcorr_", "tomography_alignment_amd/csrc/xcorr"),
    (_fbp_lib, "fbp", "tomo_fbp_", "tomography_alignment_amd/csrc/fbp"),
    (_prep_lib, "prep", "tomo_prep_", "tomography_alignment_amd/csrc/prep"),
    (_pyr_lib, "pyr", "tomo_pyr_", "tomography_alignment_amd/csrc/pyr"),
    (_fsc_lib, "fsc", "tomo_fsc_", "tomography_alignment_amd/csrc/fsc"),
    (_phase_lib, "phase", "tomo_phase_", "tomography_alignment_amd/csrc/phase"),
]
IDS = [m[1] for m in MODULES]
HANDLES = [_xcorr_lib.XcorrHandle, _fbp_lib.FbpHandle, _prep_lib.PrepHandle, _pyr_lib.PyrHandle, _fsc_lib.FscHandle, _phase_lib.PhaseHandle]


@pytest.mark.parametrize("mod,name,prefix,build_dir", MODULES, ids=IDS)
def test_load_binds_the_whole_table_once(mod, name, prefix, build_dir):
    lib = mod.load()
    assert mod.load() is lib
    assert mod.SIGNATURES
    for sym, (res, args) in mod.SIGNATURES.items():
        assert sym.startswith(prefix), sym
        fn = getattr(lib, sym)
        assert fn.restype is res and list(fn.argtypes) == list(args), sym


@pytest.mark.parametrize("mod,name,prefix,build_dir", [MODULES[0], MODULES[5], MODULES[3]], ids=["hip", "fsc", "prep"])
def test_a_missing_library_is_named_with_its_build_command(mod, name, prefix, build_dir, monkeypatch, tmp_path):
    mod.load()
    missing = str(tmp_path / ("libtomo_%s.so" % name))
    monkeypatch.setattr(mod, "LIB_PATH", missing)              # load() reads the module's LIB_PATH when it is called
    monkeypatch.delitem(_binding._loaded, name)
    with pytest.raises(_lib.TomoError) as e:
        mod.load()
    text = str(e.value)
    assert "libtomo_%s.so not built" % name in text and missing in text
    assert "`make -C %s`" % build_dir in text
    assert name not in _binding._loaded
    monkeypatch.undo()
    assert mod.load() is _binding._loaded[name]


def test_the_error_classes_are_one_family():
    assert _lib.TomoError is _binding.TomoError and issubclass(_lib.TomoError, RuntimeError)
    for cls in (_fbp_lib.FbpUnsupported, _prep_lib.PrepUnsupported, _pyr_lib.PyrUnsupported, _fsc_lib.FscUnsupported):
        assert issubclass(cls, _lib.TomoError)


def test_handle_less_calls_raise_in_the_common_format():
    with pytest.raises(_prep_lib.PrepUnsupported, match=r"^libtomo_phase error 4: tomo_phase"):
        _phase_lib.padded_length(9000, 0)
    with pytest.raises(_fsc_lib.FscUnsupported, match=r"^libtomo_fsc error 4: tomo_fsc"):
        _fsc_lib.n_shells(3, 1, 1, 8, 8)
    with pytest.raises(_lib.TomoError, match=r"^libtomo_prep error 1: tomo_prep_stripe_chunk") as e:
        _prep_lib.stripe_chunk(0, 8, 8)
    assert type(e.value) is _lib.TomoError


@pytest.mark.parametrize("cls", HANDLES, ids=[c.NAME for c in HANDLES])
def test_no_device_means_no_handle(cls):
    n = ctypes.c_int(0)
    if _lib.load().tomo_device_count(ctypes.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    h = cls.__new__(cls)
    with pytest.raises(_lib.TomoError):
        h.__init__(0)
    assert h._h is None
    h.close()
    h.close()
    with pytest.raises(_lib.TomoError, match="%s handle closed" % cls.NAME):
        h.handle
