"""TrueKNN.local_pca (tknnLocalPca, include/owlknn_pca.h) against tests/pca_spec.py: every case, through every mode, with a radius
only, k only and both, through the team walk and again through the lane kernel.

What is held to what (u = 2^-24, tol_cov and tol_centroid the derived bounds of pca_spec, E its measured solver constant):
  counts, info.total, max_row, degenerate_rows          exactly
  centroid, covariance                                  inside the derived bounds
  eigenvalues                                           |l_i - l_i(float64)| <= 3 tol_cov + E u |C|_F          (Weyl)
  the solver alone, from the device's own d_cov in      residual <= E u |C_got|_F, orthonormality defect <= E u
  float64
  the normal on the rows with a gap (pca_spec.GAP)      sin(angle to the float64 normal) <= 2 (3 tol_cov + E u |C|_F) / (l1 - l0)
                                                        (Davis-Kahan)
  the sign rule                                         recomputed in fp32 from the written normal
  the curvature                                         the header's formula on the written eigenvalues, one rounding per operation
  row 0 of the eigenvectors                             the normal, bit for bit
  degenerate rows                                       count, centroid and covariance as ever, the eigen outputs exactly 0
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import pca_spec as ps  # noqa: E402

pytestmark = pytest.mark.gpu

FALLBACK = "TKNN_PCA_FORCE_FALLBACK"
U = ps.U


@pytest.fixture(scope="module")
def eng():
    from owlraytracing_amd.trueknn import TrueKNN

    e = TrueKNN(device=0)
    yield e
    e.close()


def pca(eng, c, mode, hood, viewpoint=None, want=ps.OUTPUTS, min_points=3):
    """One call, its tensors as numpy."""
    res = eng.local_pca(radius=hood[1], k=hood[2], queries=c["Q"] if mode == "ext" else None, skip_self=mode == "own_skip", viewpoint=viewpoint,
                        min_points=min_points, want=want)
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def check(got, w, Qa, viewpoint=None, fallback=False, what=""):
    m = len(w["len"])
    solved, ln = w["solved"], w["len"]
    info = got["info"]
    # the counts and what the info says of them
    assert got["counts"].dtype == np.int32 and np.array_equal(got["counts"], w["counts"]), what + ": counts differ"
    assert info["total"] == ln.sum() and info["max_row"] == (ln.max() if m else 0) and info["degenerate_rows"] == (~solved).sum(), what
    assert not fallback or info["fallback_items"] == m, "with the fallback forced every query is the lane kernel's"
    assert info["solve_ms"] > 0 and info["walk_ms"] > 0 and info["finish_ms"] > 0
    # centroid and covariance
    err = np.abs(got["centroid"].astype(np.float64) - w["centroid"])
    assert (err <= w["tol_centroid"]).all(), "%s: centroid %g over the bound at %s" % (what, (err - w["tol_centroid"]).max(), np.unravel_index(np.argmax(err - w["tol_centroid"]), err.shape))
    err = np.abs(got["cov"].astype(np.float64) - w["cov"])
    assert (err <= w["tol_cov"][:, None]).all(), "%s: covariance %g over the bound at row %d" % (what, (err - w["tol_cov"][:, None]).max(), int(np.argmax((err - w["tol_cov"][:, None]).max(axis=1))))
    assert (got["centroid"][ln == 0] == 0).all() and (got["cov"][ln == 0] == 0).all(), "a row without neighbours: zeros"
    # degenerate rows
    for name in ("eigenvalues", "eigenvectors", "normals", "curvature"):
        assert (got[name][~solved] == 0).all(), "%s: %s of a degenerate row is 0" % (what, name)
    lam, vec, nrm = got["eigenvalues"], got["eigenvectors"], got["normals"]
    assert np.isfinite(lam).all() and np.isfinite(vec).all() and np.isfinite(got["curvature"]).all()
    # eigenvalues: ascending, inside Weyl's bound
    assert (lam[:, 0] <= lam[:, 1]).all() and (lam[:, 1] <= lam[:, 2]).all(), what + ": eigenvalues ascend"
    slack = 3.0 * w["tol_cov"] + ps.E * U * w["normF"]
    err = np.abs(lam.astype(np.float64) - w["eigenvalues"])
    assert (err[solved] <= slack[solved, None]).all(), "%s: eigenvalues %g over the bound" % (what, (err[solved] - slack[solved, None]).max())
    # the solver alone: from the device's own covariance
    if solved.any():
        dfc = ps.defects(got["cov"][solved], lam[solved], vec[solved])
        assert (dfc["residual"] <= ps.E * U).all(), "%s: residual %g u" % (what, dfc["residual"].max() / U)
        assert (dfc["ortho"] <= ps.E * U).all(), "%s: orthonormality defect %g u" % (what, dfc["ortho"].max() / U)
    # the normal where the float64 one is determined
    g = w["gap"]
    if g.any():
        sin = np.linalg.norm(np.cross(nrm[g].astype(np.float64), w["normal"][g]), axis=1)
        bound = 2.0 * slack[g] / (w["eigenvalues"][g, 1] - w["eigenvalues"][g, 0])
        assert (sin <= bound).all(), "%s: normal %g over the Davis-Kahan bound" % (what, (sin - bound).max())
    # the sign rule, the curvature, row 0 of the eigenvectors
    sign = ps.sign32(nrm, Qa, viewpoint)
    assert (sign[solved] >= 0).all() if viewpoint is not None else (sign[solved] > 0).all(), what + ": the normal's sign"
    assert np.array_equal(vec[:, 0, :].view(np.uint32), nrm.view(np.uint32)), what + ": row 0 of the eigenvectors is the normal"
    cw = ps.curvature32(lam).astype(np.float64)
    assert (np.abs(got["curvature"].astype(np.float64) - cw)[solved] <= 2.0 * U * cw[solved] + 1e-45).all(), what + ": curvature"
    assert (got["curvature"] >= 0).all() and (got["curvature"] <= np.float32(1.0 / 3.0) * (1 + 4 * U) + ps.E * U).all()


PAIRS = [(name, mode) for name in ps.CASE_NAMES for mode in (("ext",) if name == "long" else ("ext", "own", "own_skip"))]
VIEWPOINT = (0.4, 0.3, 2.5)


@pytest.mark.parametrize("name,mode", PAIRS)
def test_every_case_mode_and_neighbourhood(eng, name, mode, monkeypatch):
    c = ps.case(name)
    eng.build(c["P"], ids=c["ids"])
    Qa = c["Q"] if mode == "ext" else c["P"]
    for fallback in (False, True):
        if fallback:
            monkeypatch.setenv(FALLBACK, "1")
        for hood in c["hoods"]:
            w = ps.want_of(name, mode, hood, with_ids=c["ids"] is not None)[1]
            what = "%s %s %s%s" % (name, mode, ps.hood_label(hood), " (lane kernel)" if fallback else "")
            got = pca(eng, c, mode, hood)
            check(got, w, Qa, None, fallback, what)
            if hood is c["hoods"][0] or hood is c["hoods"][-1]:  # towards a viewpoint: the same normal up to its sign
                seen = pca(eng, c, mode, hood, viewpoint=VIEWPOINT)
                check(seen, w, Qa, VIEWPOINT, fallback, what + " oriented")
                assert np.array_equal(np.abs(seen["normals"]), np.abs(got["normals"])) and np.array_equal(seen["eigenvalues"], got["eigenvalues"])


def test_min_points_and_the_short_rows(eng):
    """Rows of 0, 1 and 2 neighbours, and min_points above and below a row's length."""
    c = ps.case("cube1025")
    eng.build(c["P"])
    for mode, k in (("ext", 1), ("ext", 2), ("own", 2), ("own_skip", 1)):
        hood = ("k", None, k)
        mem = ps.members(c["P"], c["Q"] if mode == "ext" else None, k=k, skip_self=mode == "own_skip")
        assert (mem["lengths"] == k).all()
        for min_points in (0, 1, 2, 3):
            w = ps.want(c["P"], c["Q"] if mode == "ext" else None, mem, min_points=min_points or 3)
            check(pca(eng, c, mode, hood, min_points=min_points), w, c["Q"] if mode == "ext" else c["P"], what="%s k=%d min_points=%d" % (mode, k, min_points))
    hood = ("r", np.float32(0.02), None)  # most rows are empty, the own points' hold the point alone
    for mode in ("ext", "own", "own_skip"):
        mem = ps.members(c["P"], c["Q"] if mode == "ext" else None, radius=hood[1], skip_self=mode == "own_skip")
        assert (mem["lengths"] == 0).any() or mode == "own"
        for min_points in (1, 3, 40):
            w = ps.want(c["P"], c["Q"] if mode == "ext" else None, mem, min_points=min_points)
            check(pca(eng, c, mode, hood, min_points=min_points), w, c["Q"] if mode == "ext" else c["P"], what="%s sparse min_points=%d" % (mode, min_points))


def test_every_output_alone_gives_the_same_bits(eng, monkeypatch):
    c = ps.case("plane1025")
    eng.build(c["P"])
    for fallback in (False, True):
        if fallback:
            monkeypatch.setenv(FALLBACK, "1")
        for mode, hood in (("ext", c["hoods"][0]), ("own", c["hoods"][3]), ("own_skip", c["hoods"][-1])):
            everything = pca(eng, c, mode, hood)
            for name in ps.OUTPUTS:
                alone = pca(eng, c, mode, hood, want=(name,))
                assert set(alone) == {name, "info"}
                assert alone[name].dtype == everything[name].dtype and alone[name].tobytes() == everything[name].tobytes(), (mode, name)
                assert alone["info"]["total"] == everything["info"]["total"]
            pair = pca(eng, c, mode, hood, want=("cov", "normals"), viewpoint=VIEWPOINT)
            assert pair["cov"].tobytes() == everything["cov"].tobytes() and np.array_equal(np.abs(pair["normals"]), np.abs(everything["normals"]))


@pytest.mark.parametrize("name", ("n17", "n1025"))
def test_radius_counts_are_the_lists_lengths_and_the_sums_counts(eng, name, monkeypatch):
    """With a radius only, a row's count is radius_query's row length for external queries and radius_reduce's count for the own
    points without themselves: the three calls walk alike (radius_walk.h) and differ in their rules.  At the `half` radius of
    reduce_spec's sets more boxes lie inside the sphere than a team's range list holds."""
    c = ps.rd.case(name)
    r = c["radii"]["half"]
    eng.build(c["P"])
    lengths = np.diff(eng.radius_query(c["Q"], r, sort=False, want_dist=False)["offsets"].cpu().numpy())
    sums = eng.radius_reduce(r, skip_self=True, want_wsum=False)["counts"].cpu().numpy()
    for fallback in (False, True):
        if fallback:
            monkeypatch.setenv(FALLBACK, "1")
        ext = eng.local_pca(radius=r, queries=c["Q"], want=("counts",))
        own = eng.local_pca(radius=r, skip_self=True, want=("counts",))
        assert np.array_equal(ext["counts"].cpu().numpy(), lengths), "external queries%s" % (" (lane kernel)" if fallback else "")
        assert np.array_equal(own["counts"].cpu().numpy(), sums), "own points, skip_self%s" % (" (lane kernel)" if fallback else "")
        assert ext["info"]["total"] == lengths.sum() and own["info"]["total"] == sums.sum()
        assert not fallback or (ext["info"]["fallback_items"] == len(c["Q"]) and own["info"]["fallback_items"] == len(c["P"]))


def test_normals_is_local_pca_with_three_outputs(eng):
    c = ps.case("sphere1025")
    eng.build(c["P"])
    full = eng.local_pca(k=16)
    res = eng.normals(k=16)
    assert set(res) == {"normals", "curvature", "counts", "info"}
    for name in ("normals", "curvature", "counts"):
        assert bool((res[name] == full[name]).all())
    # a sphere's normal is its radius vector: within a few degrees at 16 neighbours of 1 025 points
    radial = c["P"].astype(np.float64) - 0.5
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    cosine = np.abs((res["normals"].cpu().numpy().astype(np.float64) * radial).sum(axis=1))
    assert np.median(cosine) > 0.99
    out = eng.normals(k=16, viewpoint=(0.5, 0.5, 0.5))["normals"].cpu().numpy().astype(np.float64)
    assert ((out * radial).sum(axis=1) <= 0).all(), "seen from the centre every normal points inwards"


def test_ids_and_batches_give_what_the_plain_tree_gives(eng):
    """Values never go by id here, and labels are ignored: with ids only the ties of a kNN row can move -- the spec with those ids
    says where to --, a batched tree answers as the plain one."""
    import owlraytracing_amd

    c = ps.case("cube1025")
    n = len(c["P"])
    ids = np.roll(np.random.default_rng(77).permutation(n), 1).astype(np.int32)
    batch = np.random.default_rng(78).integers(0, 3, n).astype(np.int32)
    for mode in c["modes"]:
        Q = c["Q"] if mode == "ext" else None
        Qa = c["Q"] if mode == "ext" else c["P"]
        for hood in (c["hoods"][0], c["hoods"][3], c["hoods"][-1]):
            eng.build(c["P"], ids=ids)
            mem = ps.members(c["P"], Q, radius=hood[1], k=hood[2], skip_self=mode == "own_skip", ids=ids)
            check(pca(eng, c, mode, hood), ps.want(c["P"], Q, mem), Qa, what="ids %s %s" % (mode, ps.hood_label(hood)))
            eng.build(c["P"], batch=batch, num_batches=3)
            check(pca(eng, c, mode, hood), ps.want_of("cube1025", mode, hood)[1], Qa, what="batched %s %s" % (mode, ps.hood_label(hood)))
    # the one-shot helper takes both
    hood = c["hoods"][0]
    res = owlraytracing_amd.local_pca(c["P"], c["Q"], radius=hood[1], batch=batch)
    check(res, ps.want_of("cube1025", "ext", hood)[1], c["Q"], what="one-shot")
