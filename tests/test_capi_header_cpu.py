"""The Python binding restates include/mcamd.h by hand: 27 ctypes.Structure classes and the capi.PROTOTYPES table.  This
file parses the header and compares the two, field by field and parameter by parameter, so that a swapped pair of
fields or an int where the header says uint64_t fails here and not as a wrong price on the GPU.  It needs neither the
built library nor a GPU.

What it cannot see: whether a pointer is a device or a host pointer (the table types device memory and opaque handles
as c_void_p and host arrays as POINTER(...); the header spells both `T *`), and what any value means.

The last test pins what the binding's shared struct builders fill in and their refusals' words."""
import ctypes as C
import importlib
import os
import re

import pytest

from conftest import ROOT

capi = importlib.import_module("monte-carlo-project-cuda_amd").capi

# header struct -> binding class, and the size its C source static_asserts
STRUCTS = {
    # csrc/capi.cpp
    "mcamd_option": (capi.Option, 88), "mcamd_sim": (capi.Sim, 48), "mcamd_result": (capi.Result, 128),
    "mcamd_device_info": (capi.DeviceInfo, 384), "mcamd_greeks": (capi.Greeks, 224),
    # csrc/capi_american.cpp
    "mcamd_american": (capi.American, 32), "mcamd_american_result": (capi.AmericanResult, 152),
    "mcamd_american_dual": (capi.AmericanDual, 16), "mcamd_american_dual_result": (capi.AmericanDualResult, 104),
    # csrc/capi_pathdep.cpp
    "mcamd_barrier": (capi.Barrier, 16), "mcamd_lookback": (capi.Lookback, 16), "mcamd_asian": (capi.Asian, 24),
    # csrc/capi_multi.cpp
    "mcamd_basket": (capi.Basket, 728), "mcamd_autocall": (capi.Autocall, 632),
    "mcamd_autocall_result": (capi.AutocallResult, 112),
    # csrc/capi_localvol.cpp
    "mcamd_autocall_localvol": (capi.AutocallLocalVol, 632), "mcamd_localvol_grid": (capi.LocalVolGrid, 24),
    "mcamd_localvol": (capi.LocalVol, 24), "mcamd_localvol_greeks_job": (capi.LocalVolGreeksJob, 24),
    "mcamd_localvol_greeks": (capi.LocalVolGreeks, 472), "mcamd_cliquet": (capi.Cliquet, 56),
    "mcamd_cliquet_result": (capi.CliquetResult, 96),
    # csrc/capi_smile.cpp
    "mcamd_smile": (capi.Smile, 24),
    # csrc/capi_heston.cpp
    "mcamd_heston": (capi.Heston, 64), "mcamd_heston_result": (capi.HestonResult, 96),
    "mcamd_heston_cliquet_result": (capi.HestonCliquetResult, 112),
    "mcamd_heston_barrier_result": (capi.HestonBarrierResult, 104),
}
OPAQUE = {"mcamd_ctx", "mcamd_group", "mcamd_localvol_surface"}

# a scalar C type as (bytes, "signed" | "unsigned" | "float" | "char")
SCALARS = {"int": (4, "signed"), "int32_t": (4, "signed"), "uint32_t": (4, "unsigned"), "uint64_t": (8, "unsigned"),
           "float": (4, "float"), "double": (8, "float"), "char": (1, "char")}


def kind(ctype):
    """the same pair for a ctypes scalar type"""
    code = ctype._type_
    family = "float" if code in "fd" else "char" if code == "c" else "signed" if code in "bhilq" else "unsigned"
    assert family != "unsigned" or code in "BHILQ", ctype
    return C.sizeof(ctype), family


def is_pointer(ctype):
    return ctype in (C.c_void_p, C.c_char_p) or issubclass(ctype, C._Pointer)


def declarator(text):
    """'const double stats[6]' -> ('double', 'stats', stars 0, dims ['6'])"""
    dims = re.findall(r"\[([^\]]*)\]", text)
    words = [w for w in re.findall(r"\w+", text.split("[")[0]) if w != "const"]
    assert len(words) == 2, text
    return words[0], words[1], text.count("*"), dims


@pytest.fixture(scope="module")
def header():
    text = open(os.path.join(ROOT, "include", "mcamd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    macros = {m[0]: int(m[1]) for m in re.findall(r"^#define\s+(MCAMD_\w+)\s+(-?\d+)\s*$", text, flags=re.M)}
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    structs = {}
    for name, body, alias in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        assert name == alias, (name, alias)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            ctype, first = decl.split(None, 1)
            for item in first.split(","):
                _, field, stars, dims = declarator(ctype + " " + item)
                assert stars == 0, decl
                fields.append((field, ctype, [macros[d] if d in macros else int(d) for d in dims]))
        structs[name] = fields
    protos = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\*?)\s*\b(mcamd_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in protos, name
        params = [p.strip() for p in params.split(",")]
        protos[name] = (" ".join(ret.split()), [] if params == ["void"] else [declarator(p) for p in params])
    assert len(structs) == 27 and len(protos) == len(capi.EXPORTS) == 95, (len(structs), len(protos))
    return structs, protos


def test_the_map_names_every_struct_of_the_header_and_of_the_binding(header):
    structs, _ = header
    assert set(structs) == set(STRUCTS)
    classes = [cls for cls, _ in STRUCTS.values()]
    bound = {v for v in vars(capi).values()
             if isinstance(v, type) and issubclass(v, C.Structure) and not v.__name__.startswith("_")}
    assert len(set(classes)) == 27 and set(classes) == bound


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_fields_and_size_are_the_headers(header, name):
    structs, _ = header
    cls, size = STRUCTS[name]
    declared = structs[name]
    assert [f[0] for f in cls._fields_] == [f[0] for f in declared]
    for (field, ctype), (_, c_name, dims) in zip(cls._fields_, declared):
        got_dims = []
        while hasattr(ctype, "_length_"):
            got_dims.append(ctype._length_)
            ctype = ctype._type_
        assert got_dims == dims, (name, field)
        assert kind(ctype) == SCALARS[c_name], (name, field, c_name)
    assert C.sizeof(cls) == size


def test_exports_are_the_declared_functions(header):
    _, protos = header
    assert set(protos) == set(capi.EXPORTS) == set(capi.PROTOTYPES) and list(capi.PROTOTYPES) == capi.EXPORTS


@pytest.mark.parametrize("name", capi.EXPORTS)
def test_prototype_is_the_headers(header, name):
    _, protos = header
    ret, params = protos[name]
    restype, argtypes = capi.PROTOTYPES[name]
    assert restype is {"int": C.c_int, "float": C.c_float, "double": C.c_double, "const char *": C.c_char_p}[ret]
    assert len(argtypes) == len(params), (len(argtypes), len(params))
    for i, (got, (c_name, arg, stars, dims)) in enumerate(zip(argtypes, params)):
        where = (name, i, arg)
        levels = stars + len(dims)   # `T name[N]` is a pointer
        if levels == 0:
            assert not is_pointer(got) and kind(got) == SCALARS[c_name], where
            continue
        assert is_pointer(got), where
        if c_name in STRUCTS:
            assert levels == 1 and got is C.POINTER(STRUCTS[c_name][0]), where
        elif c_name in OPAQUE:
            assert got is (C.c_void_p if levels == 1 else C.POINTER(C.c_void_p)), where
        elif levels == 2:
            assert got is C.POINTER(C.c_void_p), where
        elif got is C.c_char_p:
            assert c_name == "char", where
        elif got is not C.c_void_p:   # a host pointer to scalars: the pointee is the header's
            assert c_name in SCALARS and kind(got._type_) == SCALARS[c_name], where
        else:
            assert c_name in SCALARS or c_name == "void", where


def test_asset_builders_fill_their_own_field_and_refuse_in_their_own_words():
    # make_autocall and make_autocall_localvol share one builder, and make_basket its correlation fill: what they leave
    # in the struct and the three refusals, word for word
    corr = [[1.0, 0.3, 0.1], [0.3, 1.0, 0.2], [0.1, 0.2, 1.0]]
    a = capi.make_autocall([0.2, 0.3, 0.4], corr, 3, 1.05, 0.02, 0.7, capi.AUTOCALL_KI_EVERY_STEP, 0.01, 2)
    b = capi.make_autocall_localvol([0.01, 0.02, 0.03], corr, 3, 1.05, 0.02, 0.7, capi.AUTOCALL_KI_EVERY_STEP, 0.01, 2)
    assert type(a) is capi.Autocall and type(b) is capi.AutocallLocalVol
    assert list(a.v) == [0.2, 0.3, 0.4] + [0.0] * 5 and list(b.q) == [0.01, 0.02, 0.03] + [0.0] * 5
    k = capi.make_basket([90.0, 100.0, 110.0], [0.2, 0.3, 0.4], [0.5, 0.25, 0.25], corr, capi.BASKET_WORST_OF,
                         capi.PAYOFF_PUT, capi.BASKET_DOWN_OUT)
    assert (k.n_assets, k.kind, k.payoff, k.barrier) == (3, capi.BASKET_WORST_OF, capi.PAYOFF_PUT, capi.BASKET_DOWN_OUT)
    assert list(k.S0)[:4] == [90.0, 100.0, 110.0, 0.0] and list(k.v)[:4] == [0.2, 0.3, 0.4, 0.0]
    assert list(k.w)[:4] == [0.5, 0.25, 0.25, 0.0]
    for s in (a, b, k):
        assert [s.corr[8 * i + j] for i in range(3) for j in range(3)] == [c for row in corr for c in row]
        assert sum(s.corr) == sum(c for row in corr for c in row)   # and nothing outside the 3 x 3 corner
    for s in (a, b):
        assert (s.n_assets, s.ki_monitoring, s.observe_every, s.first_call_date) == (3, capi.AUTOCALL_KI_EVERY_STEP, 3, 2)
        assert (s.call_level, s.call_step_down, s.coupon, s.ki_level) == (1.05, 0.01, 0.02, 0.7)
    eye9 = [[float(i == j) for j in range(9)] for i in range(9)]
    for call, text in (
            (lambda: capi.make_autocall([0.2] * 9, eye9),
             "an autocallable takes 1..8 assets, v of d and corr of d x d values"),
            (lambda: capi.make_autocall_localvol([0.0] * 2, corr),
             "an autocallable takes 1..8 assets, q of d and corr of d x d values"),
            (lambda: capi.make_basket([1.0] * 3, [1.0] * 3, [1.0] * 2, corr),
             "a basket takes 1..8 assets and S0, v, w of d and corr of d x d values")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
