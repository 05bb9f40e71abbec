"""CPU: the C ABI is declared once.  The ctypes bindings are read from include/xitorch_amd.h (`_capi.parse_prototypes`),
so these tests cover the parser on literal prototypes, the header as a whole, the loaded library against the parse, and
six signatures frozen from the hand-written table the parse replaced -- one per type class that crosses the boundary."""
import ctypes
import re
import pytest
from xitorch_amd import _capi

P, I, Lg, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double


def test_parser_cases():
    parse = _capi.parse_prototypes
    # one prototype per type spelling of the parser's table
    assert parse("int xk_a(const double* x);") == {"xk_a": (I, [P])}
    assert parse("int xk_a(void** out);") == {"xk_a": (I, [P])}
    assert parse("int xk_a(unsigned* hist16, void *stream);") == {"xk_a": (I, [P, P])}
    assert parse("int xk_a(int n);") == {"xk_a": (I, [I])}
    assert parse("int xk_a(unsigned n);") == {"xk_a": (I, [I])}
    assert parse("int xk_a(unsigned int n);") == {"xk_a": (I, [I])}
    assert parse("int xk_a(long ld);") == {"xk_a": (I, [Lg])}
    assert parse("int xk_a(double alpha);") == {"xk_a": (I, [D])}
    assert parse("int xk_a(const int n, const long ld);") == {"xk_a": (I, [I, Lg])}
    assert parse("long xk_a(int, long, double, void*);") == {"xk_a": (Lg, [I, Lg, D, P])}       # unnamed parameters
    assert parse("int xk_a(void);") == {"xk_a": (I, [])}
    assert parse("long xk_a( void );") == {"xk_a": (Lg, [])}
    # a prototype over several lines, two in one text
    multi = "int xk_ab_f64(const double* A, long lda,\n                  int B,\n   double alpha, void* stream);\nlong xk_n(void);\n"
    assert parse(multi) == {"xk_ab_f64": (I, [P, Lg, I, D, P]), "xk_n": (Lg, [])}
    # comments and preprocessor lines are no prototypes, whatever they contain
    text = "#define XK_OK 0\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n/* call xk_foo(a, b) first;\n * int xk_bar(int x); */\nint xk_a(int n);\n"
    assert parse(text) == {"xk_a": (I, [I])}
    # a type the boundary does not carry raises and names the function and the parameter
    for bad in ("float x", "struct s v", "long long n", "unsigned long n", "char c", "size_t n"):
        with pytest.raises(_capi.NativeLibraryError) as e:
            parse("int xk_a(int n, %s);" % bad)
        assert "xk_a" in str(e.value) and bad in str(e.value)
    with pytest.raises(_capi.NativeLibraryError):
        parse("int xk_a();")                                  # not a prototype in C: `(void)` is spelled out
    # an xk_ name whose declaration the parser does not understand is an error, not an unbound function
    for shape in ("void xk_a(int n);", "int xk_a(int (*cb)(int), int n);", "static inline int xk_a(int n) { return n; }",
                  "unsigned xk_a(int n);"):
        with pytest.raises(_capi.NativeLibraryError) as e:
            parse("int xk_ok(void);\n" + shape)
        assert "xk_a" in str(e.value) and "xk_ok" not in str(e.value)


def test_every_name_in_the_header_has_a_parsed_prototype():
    txt = re.sub(r"/\*.*?\*/", "", open(_capi.HEADER_PATH).read(), flags=re.S)
    loose = set(re.findall(r"\b(xk_[a-z0-9_]+)\s*\(", txt))
    sigs = _capi.signatures()
    assert set(sigs) == loose
    assert _capi.header_symbols() == sorted(loose)
    assert len(loose) >= 184
    assert all(res in (I, Lg) for res, _ in sigs.values())


def test_loaded_library_is_typed_by_the_parse():
    L = _capi.lib()
    for name, (res, args) in _capi.signatures().items():
        assert hasattr(L, name), name
        f = getattr(L, name)
        assert f.restype is res, name
        assert f.argtypes is not None and list(f.argtypes) == args, name


def test_frozen_signatures():
    """literals from the table `_declare` held before it read the header: one per type class"""
    frozen = {
        "xk_dense_mm_f64": (I, [P, P, P, P, Lg, I, I, I, I, Lg, Lg, Lg, Lg, Lg, Lg, I, I, I, P]),
        "xk_dense_mm_workspace_elems": (Lg, [I, I, I, I, I]),                                       # long return
        "xk_lincomb_c64": (I, [P, P, P, I, I, I, I, Lg, Lg, Lg, Lg, Lg, Lg, D, D, P]),              # double by value
        "xk_probe_xcc": (I, [P, P, I, I, P]),                                                       # unsigned*
        "xk_stream_create_cu_masked": (I, [I, I, P]),                                               # void**
        "xk_kry_max_partials": (I, []),                                                             # (void)
    }
    sigs = _capi.signatures()
    for name, sig in frozen.items():
        assert sigs[name] == sig, name
