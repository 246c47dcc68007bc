"""include/mcamd_heston_greeks.h against its binding, monte-carlo-project-cuda_amd/heston_greeks.py: the two structs field
by field and the four prototypes parameter by parameter, the way tests/test_capi_header_cpu.py compares mcamd.h with
capi.py (whose helpers and struct map this file borrows), and every declared function as a defined dynamic symbol of
the built library.  It also pins what keeps the two headers apart: mcamd.h and capi's tables do not know these names."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_capi_header_cpu import OPAQUE, SCALARS, STRUCTS as CAPI_STRUCTS, declarator, is_pointer, kind

pkg = importlib.import_module("monte-carlo-project-cuda_amd")
capi = pkg.capi
hg = importlib.import_module("monte-carlo-project-cuda_amd.heston_greeks")

# header struct -> binding class, and the size csrc/capi_heston.cpp static_asserts
STRUCTS = {"mcamd_heston_greeks_job": (hg.HestonGreeksJob, 56), "mcamd_heston_greeks": (hg.HestonGreeks, 208)}
KNOWN = dict(CAPI_STRUCTS, **STRUCTS)


def raw():
    with open(os.path.join(ROOT, "include", "mcamd_heston_greeks.h")) as f:
        return f.read()


@pytest.fixture(scope="module")
def header():
    text = re.sub(r"/\*.*?\*/", " ", raw(), flags=re.S)
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
        protos[name] = (" ".join(ret.split()), [declarator(p.strip()) for p in params.split(",")])
    assert len(structs) == 2 and len(protos) == len(hg.EXPORTS) == 4, (len(structs), len(protos))
    return structs, protos, macros


def test_the_map_names_every_struct_of_the_header_and_of_the_binding(header):
    structs, _, _ = header
    assert set(structs) == set(STRUCTS)
    bound = {v for v in vars(hg).values() if isinstance(v, type) and issubclass(v, C.Structure)}
    assert bound == {cls for cls, _ in STRUCTS.values()}
    # capi keeps the structs of mcamd.h and no other: these two live here alone
    assert not any(isinstance(v, type) and issubclass(v, C.Structure) and v.__name__.startswith("HestonGreeks")
                   for v in vars(capi).values())


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_fields_and_size_are_the_headers(header, name):
    structs, _, _ = header
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
    with open(os.path.join(ROOT, "monte-carlo-project-cuda_amd", "csrc", "capi_heston.cpp")) as f:
        assert re.search(r"sizeof\(" + name + r"\) == " + str(size) + r"\b", f.read())


def test_exports_are_the_declared_functions(header):
    _, protos, _ = header
    assert set(protos) == set(hg.EXPORTS) == set(hg.PROTOTYPES) and list(hg.PROTOTYPES) == hg.EXPORTS
    # the set of mcamd_...( names anywhere in the header's text, comments included, beyond mcamd.h's own
    named = {n[:-1] for n in re.findall(r"mcamd_[a-z0-9_]+\(", raw())}
    assert named - set(capi.EXPORTS) == set(hg.EXPORTS), named - set(capi.EXPORTS)
    assert not set(hg.EXPORTS) & set(capi.EXPORTS)
    with open(os.path.join(ROOT, "include", "mcamd.h")) as f:
        assert "heston_greeks" not in f.read()


@pytest.mark.parametrize("name", hg.EXPORTS)
def test_prototype_is_the_headers(header, name):
    _, protos, _ = header
    ret, params = protos[name]
    restype, argtypes = hg.PROTOTYPES[name]
    assert restype is {"int": C.c_int}[ret]
    assert len(argtypes) == len(params), (len(argtypes), len(params))
    for i, (got, (c_name, arg, stars, dims)) in enumerate(zip(argtypes, params)):
        where = (name, i, arg)
        levels = stars + len(dims)   # `T name[N]` is a pointer
        if levels == 0:
            assert not is_pointer(got) and kind(got) == SCALARS[c_name], where
            continue
        assert is_pointer(got) and levels == 1, where
        if c_name in KNOWN:
            assert got is C.POINTER(KNOWN[c_name][0]), where
        elif c_name in OPAQUE:
            assert got is C.c_void_p, where
        elif got is not C.c_void_p:   # a host pointer to scalars: the pointee is the header's
            assert c_name in SCALARS and kind(got._type_) == SCALARS[c_name], where
        else:
            assert c_name in SCALARS or c_name == "void", where


def test_macros_are_the_bindings(header):
    _, _, macros = header
    names = ("PRICE", "DELTA", "GAMMA", "RHO", "RHO_Q", "V0", "KAPPA", "THETA", "XI", "CORR")
    assert [macros["MCAMD_HESTON_GREEK_" + n] for n in names] == list(range(10))
    assert [getattr(hg, "GREEK_" + n) for n in names] == list(range(10))
    assert macros["MCAMD_HESTON_GREEKS"] == hg.GREEKS == len(hg.GREEK_NAMES) == 10
    assert macros["MCAMD_HESTON_GREEKS_STATS"] == hg.STATS == 32
    text = re.sub(r"\s*\n \*\s*", " ", raw())   # the comment's lines joined
    assert '#include "mcamd.h"' in text and "Additive to ABI version 5" in text
    assert "first carried by the build that ships csrc/heston_greeks.hip" in text
    assert not re.search(r"mcamd_group_\w*heston", text)


def test_the_job_builder_fills_the_fields_in_the_headers_order():
    j = hg.make_job(0.01, v0=1.0, kappa=2.0, theta=3.0, xi=4.0, rho=5.0)
    assert (j.gamma_eta, list(j.bump), j.reserved) == (0.01, [1.0, 2.0, 3.0, 4.0, 5.0], 0.0) and hg.PARAMS == (
        "v0", "kappa", "theta", "xi", "rho")
    assert (j.n_params, j.n_rows) == (5, 13)
    k = hg.make_job(xi=0.05)
    assert (k.gamma_eta, list(k.bump), k.n_params, k.n_rows) == (0.0, [0.0, 0.0, 0.0, 0.05, 0.0], 1, 5)
    assert (hg.make_job().n_params, hg.make_job().n_rows) == (0, 3)


def test_every_declared_function_is_a_defined_dynamic_symbol_and_the_build_knows_the_files():
    if not os.path.exists(capi.LIB_PATH):
        pkg.build()
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.check_output([nm, "-D", "--defined-only", capi.LIB_PATH], text=True)
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [name for name in hg.EXPORTS if name not in defined]
    L = hg.load()
    assert all(getattr(L, name).argtypes == hg.PROTOTYPES[name][1] for name in hg.EXPORTS)
    build = importlib.import_module("monte-carlo-project-cuda_amd.build")
    assert "heston_greeks.hip" in build.SOURCES and "heston_greeks.hpp" in build.HEADERS
    assert "mcamd_heston_greeks.h" in build.PUBLIC_HEADERS
    # the public header is part of the build id: another text, another id
    path = os.path.join(ROOT, "include", "mcamd_heston_greeks.h")
    real_open, before = open, build.build_id()

    def patched(file, *a, **kw):
        f = real_open(file, *a, **kw)
        if os.path.abspath(str(file)) == path and "b" in (a[0] if a else kw.get("mode", "r")):
            import io
            return io.BytesIO(f.read() + b"\n")
        return f
    build.open = patched
    try:
        assert build.build_id() != before
    finally:
        del build.open
    assert build.build_id() == before
