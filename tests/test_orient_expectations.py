"""The spec of tknnOrientNormals (tests/orient_spec.py) held to what it claims, without a GPU: its two computations of the flips agree,
a sphere's radial normals come out outward whatever their signs were, the result does not depend on the input's signs, the spec's own
output is a fixed point, and the ctypes records of owlraytracing_amd/_orient_lib.py have the header's layout."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import orient_spec as osp  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", osp.SMALL + ("sphere_noisy", "lattice", "direction_tie", "two_spheres_no_emst"))
def test_the_two_flip_computations_agree(name):
    c, want = osp.case(name)  # (orient() asserts it; here it is seen to have run, on every component)
    assert np.array_equal(want["flip"], want["flip_dfs"]) and len(want["roots"]) == want["components"]
    ok = osp.eligible(c["P"], c["N"])
    assert want["excluded"] == (~ok).sum() and (want["flip"][~ok] == 0).all() and (want["component"][~ok] == -1).all()
    assert np.array_equal(bits(want["normals"])[~ok], bits(c["N"])[~ok]), "a point left out keeps its normal, bit for bit"
    assert want["tree_edges"] == ok.sum() - want["components"] and (want["u"] < want["v"]).all()
    key = list(zip(want["w"].view(np.uint32).tolist(), want["u"].tolist(), want["v"].tolist()))
    assert key == sorted(key) and len(set(key)) == len(key), "records ascend by the strict key"


def test_the_cases_are_what_they_say():
    assert osp.case("two_spheres_no_emst")[1]["components"] == 2 and len(osp.case("two_spheres_no_emst")[1]["roots"]) == 2
    assert osp.case("two_spheres")[1]["components"] == 1
    c, want = osp.case("direction_tie")
    t = osp.dot3(c["P"], np.float32(c["direction"])[None, :])
    assert (t == t.max()).sum() == 144 and want["roots"].tolist() == [int(np.flatnonzero(t == t.max()).min())]
    c, want = osp.case("plane_ids_above_n")
    assert (want["w"].view(np.uint32) == 0).all() and want["roots"].tolist() == [0] and want["flipped"] == 0 and c["ids"].min() >= len(c["P"])
    c, want = osp.case("bad_inputs")
    assert want["excluded"] == 23 + 20 and (c["N"] == 0).all(axis=1).sum() == 20
    zero = (c["N"] == 0).all(axis=1)
    assert (want["component"][zero] >= 0).all() and (want["normals"][zero] == 0).all(), "a zero normal takes part and stays zero"
    for n in osp.TINY_N:
        assert osp.case("tiny%d_kbig" % n)[0]["k"] >= n - 1 and osp.case("tiny%d_k1" % n)[0]["k"] == 1
    assert osp.case("tiny1_k1")[1]["tree_edges"] == 0 and osp.case("tiny1_k1")[1]["components"] == 1


@pytest.mark.parametrize("name", ["sphere", "two_spheres_no_emst"])
def test_a_sphere_comes_out_outward(name):
    """A property of the scene: every tree edge joins two points whose outward normals have a positive dot, and the root -- the top
    of a sphere -- has an outward normal with a positive z."""
    c, want = osp.case(name)
    assert np.array_equal(bits(want["normals"]), bits(c["outward"])), "the outward normals, bit for bit"
    assert want["flipped"] == (bits(c["N"]) != bits(c["outward"])).any(axis=1).sum() > 0


def test_two_spheres_joined_by_the_emst_are_each_consistent():
    """The one EMST record between the spheres joins their nearest points, whose outward normals oppose each other: the sphere without
    the root comes out inward as a whole -- consistent, which is all a tree can promise across such an edge."""
    c, want = osp.case("two_spheres")
    same = (bits(want["normals"]) == bits(c["outward"])).all(axis=1)
    opposite = (bits(want["normals"]) == bits(-c["outward"])).all(axis=1)
    root = int(want["roots"][0])
    a = np.arange(len(same)) < 1000
    assert same[a == a[root]].all() and opposite[a != a[root]].all()


@pytest.mark.parametrize("name", osp.SIGN_FREE)
def test_the_output_does_not_depend_on_the_input_signs(name):
    """Where no dot along the tree or at a root is exactly zero (a zero dot carries no sign: the child goes with its parent, whichever
    way the input pointed): orient_spec.SIGN_FREE names such cases."""
    c, want = osp.case(name)
    rng = np.random.default_rng(5)
    for share in (0.5, 1.0, 0.02):
        neg = rng.random(len(c["N"])) < share
        N = np.where(neg[:, None], -c["N"], c["N"]).astype(np.float32)
        got = osp.orient(c["P"], N, c["k"], ids=c["ids"], direction=c["direction"], emst=c["emst"], key=c["key"])
        ok = osp.eligible(c["P"], c["N"])
        assert np.array_equal(bits(got["normals"])[ok], bits(want["normals"])[ok]), "w uses |c| and negation is exact"
        assert np.array_equal(bits(got["normals"])[~ok], bits(N)[~ok])
        for key in ("u", "v", "component"):
            assert np.array_equal(got[key], want[key])
        assert np.array_equal(got["w"].view(np.uint32), want["w"].view(np.uint32))
        assert np.array_equal(got["flip"].astype(bool), want["flip"].astype(bool) ^ (neg & ok))


@pytest.mark.parametrize("name", ["sphere_noisy", "bad_inputs", "lattice"])
def test_the_spec_on_its_own_output_flips_nothing(name):
    c, want = osp.case(name)
    again = osp.orient(c["P"], want["normals"], c["k"], ids=c["ids"], direction=c["direction"], emst=c["emst"], key=c["key"])
    assert again["flipped"] == 0 and np.array_equal(bits(again["normals"]), bits(want["normals"]))


def test_records_have_the_headers_sizes(tmp_path):
    from owlraytracing_amd import _lib, _orient_lib

    pairs = {"tknnOrientOptions": _orient_lib.OrientOptions, "tknnOrientInfo": _orient_lib.OrientInfo}
    mirrors = {c for c in vars(_orient_lib).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and getattr(c, "_fields_", None)}
    assert mirrors == set(pairs.values())
    consts = {"TKNN_ORIENT_NO_EMST": _orient_lib.ORIENT_NO_EMST}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "owlknn_orient.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    for cname in consts:
        lines.append('  printf("const %s %%ld\\n", (long)%s);' % (cname, cname))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = 0
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, what, value = line.split()
        if cname == "const":
            assert consts[what] == int(value), what
        elif what == "size":
            assert ctypes.sizeof(pairs[cname]) == int(value), cname
        else:
            assert getattr(pairs[cname], what).offset == int(value), (cname, what)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in pairs.values()) + len(consts)
    assert ctypes.sizeof(_orient_lib.OrientOptions) == 80 and ctypes.sizeof(_orient_lib.OrientInfo) == 72
    res, args = _orient_lib.SIGNATURES["tknnOrientNormals"]
    lib = _orient_lib.load()
    assert lib is _lib.load() and lib.tknnOrientNormals.restype is res is ctypes.c_int and lib.tknnOrientNormals.argtypes == args
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT tknnOrientNormals$", exported, flags=re.M), "the library exports the symbol"
