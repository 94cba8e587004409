"""Every native library of __graft_entry__.LIBRARIES against its header and through the shared binding layer
(tomography_alignment_amd/_binding.py): the header (read by tests/abi.py) is the ctypes table -- functions, the type of every argument,
mirrored constants and structs -- and load(), the error classes and the handles behave alike.  Needs the built libraries, no GPU; the
tests of the reader itself need neither."""
import ctypes

import pytest

import abi

from tomography_alignment_amd import _binding, _fsc_lib, _lib, _phase_lib, _prep_lib

LIBS = abi.libraries()
IDS = [lib.name for lib in LIBS]
SIDE = [lib for lib in LIBS if lib.handle is not None]
every_library = pytest.mark.parametrize("lib", LIBS, ids=IDS)

# functions each header declares
N_FUNCTIONS = dict(hip=84, xcorr=11, fbp=6, prep=14, pyr=7, fsc=13, phase=11, cor=14, mom=11, dff=16, half=16, vol=14, vreg=15, seg=13,
                   morph=17, mesh=8)
# the constants a binding module mirrors under the header's name less its TOMO_<NAME>_: each must be in both and equal
MIRRORED = dict(
    hip="POSE_STRIDE GEOM_WIDE_ROWS COMM_ID_BYTES",
    xcorr="",
    fbp="ERR_UNSUPPORTED",
    prep="MAX_NPROJ MAX_MEDIAN_FRAMES MAX_STRIPE_SIZE MIN_STRIPE_NDX MAX_STRIPE_NDX MIN_DEAD_NPROJ MAX_OUTLIER_SIZE ERR_UNSUPPORTED U16 F32 MEAN "
         "MEDIAN OUTLIER MEDIAN2D",
    pyr="MAX_FACTOR ERR_UNSUPPORTED",
    fsc="MAX_N MAX_PLANES ERR_UNSUPPORTED MASK_NONE MASK_ARRAY MASK_SPHERE",
    phase="MAX_P MAX_STRENGTH ERR_UNSUPPORTED",
    cor="MIN_N MIN_NX MAX_NX MAX_R MAX_SLICES ERR_UNSUPPORTED",
    mom="MAX_NZ TILE_X CHUNK_Z ERR_UNSUPPORTED",
    dff="MAX_FLATS MAX_EFF MAX_BIN TILE_Z TILE_X MAX_IDS ERR_UNSUPPORTED U16 F32",
    half="MAX_N MIN_NX MAX_NX MAX_NZ MAX_ROWS MIN_W TILE_J TILE_P TILE_C ERR_UNSUPPORTED A_VALID B_VALID",
    vol="MAX_DIM MAX_NZ MAX_BINS SPAN_GROUPS TILE ERR_UNSUPPORTED",
    vreg="MAX_N MAX_UPSAMPLE ERR_UNSUPPORTED MASK_NONE MASK_ARRAY MASK_SPHERE NORM_NONE NORM_PHASE",
    seg="MAX_DIM MAX_VOXELS TILE_X TILE_Y TILE_Z SPAN_GROUPS KEEP_BYTES DEFAULT_SCRATCH ERR_UNSUPPORTED",
    morph="MAX_DIM MAX_VOXELS INF W MAX_WQ GROUP LINE_LIMIT KEEP_BYTES ERR_UNSUPPORTED",
    mesh="MAX_DIM MAX_VOXELS MAX_TRIANGLES GROUP KEEP_BYTES F32 U8 ERR_UNSUPPORTED ERR_CAPACITY",
)
# library, its ctypes.Structure, the header's typedef
STRUCTS = [("hip", "TomoGeom", "tomo_geom"), ("half", "Column", "tomo_half_column"), ("vol", "StatsStruct", "tomo_vol_stats_t")]


# ------------------------------------------------------------------------------------------------------------ the header is the table

@every_library
def test_the_table_is_the_header(lib):
    declared = abi.parse_header(lib.header).functions
    table = lib.module.SIGNATURES
    assert set(declared) == set(table), set(declared) ^ set(table)
    assert len(declared) == N_FUNCTIONS[lib.name]
    differences = dict((name, d) for name, d in ((name, abi.compare_signature(declared[name], table[name])) for name in declared) if d)
    assert not differences, differences


@every_library
def test_mirrored_constants_are_the_headers(lib):
    constants = abi.parse_header(lib.header).constants
    stem = lib.prefix.upper()
    assert all(name.startswith(stem) for name in constants), [name for name in constants if not name.startswith(stem)]
    for name in MIRRORED[lib.name].split():
        assert stem + name in constants, "%s%s is not in %s" % (stem, name, lib.header)
        assert hasattr(lib.module, name), "%s has no %s" % (lib.module.__name__, name)
    mirrored = [name[len(stem):] for name in constants if hasattr(lib.module, name[len(stem):])]
    assert sorted(mirrored) == sorted(MIRRORED[lib.name].split())           # a new mirrored constant joins the table above
    for name in mirrored:
        assert getattr(lib.module, name) == constants[stem + name], name


@pytest.mark.parametrize("name,struct,typedef", STRUCTS, ids=[s[2] for s in STRUCTS])
def test_mirrored_structs_are_the_headers(name, struct, typedef):
    lib = LIBS[IDS.index(name)]
    assert abi.compare_struct(abi.parse_header(lib.header).structs[typedef], getattr(lib.module, struct)) == []


# ----------------------------------------------------------------------------------------------------------- the shared binding layer

@every_library
def test_load_binds_the_whole_table_once(lib):
    so = lib.module.load()
    assert lib.module.load() is so
    assert lib.module.SIGNATURES
    for sym, (res, args) in lib.module.SIGNATURES.items():
        assert sym.startswith(lib.prefix), sym
        fn = getattr(so, sym)
        assert fn.restype is res and list(fn.argtypes) == list(args), sym
    if lib.handle is not None:
        assert lib.handle.NAME == lib.name and issubclass(lib.handle, _binding.Handle)


@every_library
def test_every_declared_symbol_is_exported(lib):
    raw = ctypes.CDLL(lib.module.LIB_PATH)                     # the library itself, whatever the table says
    for sym in abi.parse_header(lib.header).functions:
        assert hasattr(raw, sym), sym
    assert getattr(lib.module.load(), lib.prefix + "abi_version")() == 1


@every_library
def test_a_missing_library_is_named_with_its_build_command(lib, monkeypatch, tmp_path):
    mod, name = lib.module, lib.name
    mod.load()
    missing = str(tmp_path / ("libtomo_%s.so" % name))
    monkeypatch.setattr(mod, "LIB_PATH", missing)              # load() reads the module's LIB_PATH when it is called
    monkeypatch.delitem(_binding._loaded, name)
    with pytest.raises(_lib.TomoError) as e:
        mod.load()
    text = str(e.value)
    assert "libtomo_%s.so not built" % name in text and missing in text
    assert "`make -C %s`" % lib.build_dir in text
    assert name not in _binding._loaded
    monkeypatch.undo()
    assert mod.load() is _binding._loaded[name]


def test_the_error_classes_are_one_family():
    assert _lib.TomoError is _binding.TomoError and issubclass(_lib.TomoError, RuntimeError)
    own = [cls for lib in LIBS for cls in lib.errors]
    assert len([cls for cls in own if cls.__name__.endswith("Unsupported")]) == 13       # all but hip and xcorr, and phase raises prep's
    for lib in LIBS:
        mapped = list(getattr(lib.module, "ERRORS", {}).values()) + (list(lib.handle.ERRORS.values()) if lib.handle else [])
        for cls in list(lib.errors) + mapped:
            assert issubclass(cls, _lib.TomoError) and cls is not _lib.TomoError, cls


def test_handle_less_calls_raise_in_the_common_format():
    with pytest.raises(_prep_lib.PrepUnsupported, match=r"^libtomo_phase error 4: tomo_phase"):
        _phase_lib.padded_length(9000, 0)
    with pytest.raises(_fsc_lib.FscUnsupported, match=r"^libtomo_fsc error 4: tomo_fsc"):
        _fsc_lib.n_shells(3, 1, 1, 8, 8)
    with pytest.raises(_lib.TomoError, match=r"^libtomo_prep error 1: tomo_prep_stripe_chunk") as e:
        _prep_lib.stripe_chunk(0, 8, 8)
    assert type(e.value) is _lib.TomoError


@pytest.mark.parametrize("cls", [lib.handle for lib in SIDE], ids=[lib.name for lib in SIDE])
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


# ------------------------------------------------------------------------------------- the reader and the comparisons can fail (CPU only)

HEADER = """
/* A header of the package's kind; this comment holds commas, (parentheses) and a declaration:
 * TOMO_API int tomo_t_not_declared(int a, int b); */
#ifndef TOMO_T_H
#define TOMO_T_H
#if defined(TOMO_T_BUILD)
#define TOMO_API __attribute__((visibility("default")))
#else
#define TOMO_API
#endif
#define TOMO_T_MAX_N 65536          /* rows (of one call), at most */
#define TOMO_T_KEEP_BYTES (16 << 20)
#define TOMO_T_MAX_VOXELS 2147483647
#define TOMO_T_MAX_STRENGTH 1e6f    // a float
#define TOMO_T_MASK 0x10u
#define TOMO_T_NAME "t"
#define TOMO_T_TWICE (2 * TOMO_T_MAX_N)
typedef enum {
    TOMO_T_OK = 0,
    TOMO_T_ERR_UNSUPPORTED = 4      /* a size, (too large) */
} tomo_t_status;
enum { TOMO_T_A_VALID = 1, TOMO_T_B_VALID = 2 };
typedef struct {
    int flags, ja;
    float w[3];                     /* 1 - f, f, wA */
    double c;
} tomo_t_column;
typedef struct tomo_t tomo_t;
TOMO_API int tomo_t_abi_version(void);
TOMO_API const char *tomo_t_last_error(tomo_t *h);
TOMO_API int tomo_t_create(int device, tomo_t **h);
/* d_in: n values on the device, (read, not written) */
TOMO_API int tomo_t_run(tomo_t *h, void *stream, const float *d_in, size_t bytes,      /* bytes, (of d_in) */
                        int64_t n, double scale, double origin[3],
                        const tomo_t_column *columns, double *sum);
#endif
"""


class _Column(ctypes.Structure):
    _fields_ = [("flags", ctypes.c_int), ("ja", ctypes.c_int), ("w", ctypes.c_float * 3), ("c", ctypes.c_double)]


_vp, _int, _dp = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)
RUN = [_vp, _vp, _vp, ctypes.c_size_t, ctypes.c_int64, ctypes.c_double, _dp, ctypes.POINTER(_Column), _dp]


def test_the_reader_reads_a_header():
    h = abi.parse_text(HEADER)
    assert dict(h.functions) == {
        "tomo_t_abi_version": (("int", 0), []),
        "tomo_t_last_error": (("char", 1), [("tomo_t", 1)]),
        "tomo_t_create": (("int", 0), [("int", 0), ("tomo_t", 2)]),
        "tomo_t_run": (("int", 0), [("tomo_t", 1), ("void", 1), ("float", 1), ("size_t", 0), ("int64_t", 0), ("double", 0), ("double", 1),
                                    ("tomo_t_column", 1), ("double", 1)]),
    }
    assert dict(h.constants) == dict(TOMO_T_MAX_N=65536, TOMO_T_KEEP_BYTES=16 << 20, TOMO_T_MAX_VOXELS=2 ** 31 - 1, TOMO_T_MAX_STRENGTH=1e6,
                                     TOMO_T_MASK=16, TOMO_T_OK=0, TOMO_T_ERR_UNSUPPORTED=4, TOMO_T_A_VALID=1, TOMO_T_B_VALID=2)
    assert dict(h.structs) == {"tomo_t_column": [("flags", "int", None), ("ja", "int", None), ("w", "float", 3), ("c", "double", None)]}


def test_a_correct_table_has_no_differences():
    h = abi.parse_text(HEADER)
    table = {"tomo_t_abi_version": (_int, []), "tomo_t_last_error": (ctypes.c_char_p, [_vp]),
             "tomo_t_create": (_int, [_int, ctypes.POINTER(_vp)]), "tomo_t_run": (_int, RUN)}
    for name, decl in h.functions.items():
        assert abi.compare_signature(decl, table[name]) == [], name
    every_pointer_as_void_p = [_vp, _vp, _vp, ctypes.c_size_t, ctypes.c_int64, ctypes.c_double, _vp, _vp, _vp]
    assert abi.compare_signature(h.functions["tomo_t_run"], (_int, every_pointer_as_void_p)) == []
    assert abi.compare_struct(h.structs["tomo_t_column"], _Column) == []


def _run_with(i, ctype):
    return (_int, RUN[:i] + [ctype] + RUN[i + 1:])


@pytest.mark.parametrize("name,sig", [
    ("tomo_t_run", _run_with(3, _int)),                                  # c_int for size_t
    ("tomo_t_run", _run_with(5, _int)),                                  # c_int for double
    ("tomo_t_run", _run_with(4, _int)),                                  # c_int for int64_t
    ("tomo_t_run", _run_with(8, ctypes.POINTER(ctypes.c_float))),        # POINTER(c_float) for double *
    ("tomo_t_run", (_int, RUN[:-1])),                                    # one argument too few
    ("tomo_t_last_error", (_int, [_vp])),                                # c_int where const char * is returned
    ("tomo_t_create", (_int, [_int, _vp])),                              # tomo_t ** is not a tomo_t *
    ("tomo_t_abi_version", (None, [])),                                  # an int is returned
], ids=["size_t", "double", "int64_t", "double-pointer", "arity", "char-pointer-returned", "pointer-to-handle", "void-returned"])
def test_a_wrong_table_is_one_difference(name, sig):
    differences = abi.compare_signature(abi.parse_text(HEADER).functions[name], sig)
    assert len(differences) == 1, differences


def test_a_wrong_struct_is_reported():
    fields = abi.parse_text(HEADER).structs["tomo_t_column"]

    class Swapped(ctypes.Structure):
        _fields_ = [("ja", ctypes.c_int), ("flags", ctypes.c_int), ("w", ctypes.c_float * 3), ("c", ctypes.c_double)]

    class Narrow(ctypes.Structure):
        _fields_ = [("flags", ctypes.c_int), ("ja", ctypes.c_int), ("w", ctypes.c_float * 3), ("c", ctypes.c_float)]

    class Short(ctypes.Structure):
        _fields_ = [("flags", ctypes.c_int), ("ja", ctypes.c_int), ("w", ctypes.c_float * 2), ("c", ctypes.c_double)]

    for wrong in (Swapped, Narrow, Short):
        assert len(abi.compare_struct(fields, wrong)) == 1, wrong.__name__
