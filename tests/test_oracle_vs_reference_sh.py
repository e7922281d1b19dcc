"""Pins the oracle's SH restatement against REFERENCE-AUTHORED code: cugs::evaluate_sh_cpu
(src/core/sh.cpp:8-87), and against the reference's own SH tests (tests/test_sh.cpp:16-143).

The reference's answers are recorded in tests/golden/reference/sh.npz (outputs only; the inputs are re-made from the
seeds below), so the suite needs no reference tree.  Where oracle/Makefile has compiled the reference file in place
into oracle/_ref/libref_sh.so, every recorded answer is also checked against that live build.  Re-record there with
    python tests/test_oracle_vs_reference_sh.py"""
import os

import numpy as np
import pytest

C0 = 0.28209479177387814
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference", "sh.npz")
DEGREES, SIZES = (0, 1, 2, 3), (1, 200, 10_000)
BAD_INPUTS = ((4, 4), (2, 4), (1, 4))            # (degree, coefficients stored): test_sh.cpp:127-143


def _eval_inputs(degree, n):
    rng = np.random.default_rng(100 * degree + n)
    sh = rng.standard_normal((n, 3, 16)).astype(np.float32)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return sh, d


def _kat_cases():
    """name -> (degree, sh, dirs): the inputs of test_sh.cpp:16-125 as test_reference_kats_hold_for_both uses them."""
    sh = np.zeros((1, 3, 16), np.float32)
    sh[0, :, 0] = [1.0, 0.5, -0.25]
    d = np.array([[0.0, 0.0, 1.0]], np.float32)
    sh1 = np.zeros((1, 3, 16), np.float32)
    sh1[0, :, 1] = 1.0
    rng = np.random.default_rng(4)
    shb = rng.standard_normal((5, 3, 16)).astype(np.float32)
    db = rng.standard_normal((5, 3)).astype(np.float32)
    db /= np.linalg.norm(db, axis=1, keepdims=True)
    cases = {"dc": (0, sh, d), "dc_x": (0, sh, np.array([[1.0, 0.0, 0.0]], np.float32)),
             "y1_up": (1, sh1, np.array([[0.0, 1.0, 0.0]], np.float32)),
             "y1_down": (1, sh1, np.array([[0.0, -1.0, 0.0]], np.float32)),
             "deg3_dc_only": (3, sh, d), "batch": (3, shb, db)}
    for i in range(5):
        cases[f"batch_item{i}"] = (3, shb[i:i + 1], db[i:i + 1])
    return cases


def _record_all(evaluate):
    """Every answer of the reference the tests below use, by name; evaluate(degree, sh, dirs) -> (rc, rgb)."""
    rec = {}
    for degree in DEGREES:
        for n in SIZES:
            rc, rgb = evaluate(degree, *_eval_inputs(degree, n))
            assert rc == 0
            rec[f"eval_d{degree}_n{n}"] = rgb
    for name, (degree, sh, d) in _kat_cases().items():
        rc, rgb = evaluate(degree, sh, d)
        assert rc == 0
        rec["kat_" + name] = rgb
    rec["validation_rc"] = np.array([evaluate(deg, np.zeros((2, 3, c), np.float32), np.zeros((2, 3), np.float32))[0]
                                     for deg, c in BAD_INPUTS], np.int32)
    return rec


@pytest.fixture(scope="module")
def ref(orc):
    """The reference's recorded answers; checked bit for bit against the live build where oracle/_ref has one."""
    with np.load(GOLDEN) as z:
        rec = {k: z[k] for k in z.files}
    if orc.ref_sh_available():
        live = _record_all(orc.ref_evaluate_sh_cpu)
        assert set(live) == set(rec)
        for k, v in live.items():
            assert v.dtype == rec[k].dtype and np.array_equal(v, rec[k]), k
    return rec


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 200, 10_000])
def test_oracle_sh_equals_reference_cpu(ref, orc, degree, n):
    sh, d = _eval_inputs(degree, n)
    want = ref[f"eval_d{degree}_n{n}"]
    assert want.shape == (n, 3)
    got = orc.sh_forward(degree, sh, d)
    # the reference's own CUDA==CPU bar is rtol=atol=1e-4 (test_sh.cpp:161-216); the restatement
    # follows the same association so it is far tighter (g++ may contract differently: allow 1e-6)
    assert np.allclose(got, want, rtol=1e-6, atol=1e-6)


def test_reference_kats_hold_for_both(ref, orc):
    """test_sh.cpp:16-125 known answers, on the reference's recorded answers AND the oracle."""
    cases = _kat_cases()
    for evaluate in (lambda name: ref["kat_" + name], lambda name: orc.sh_forward(*cases[name])):
        sh = cases["dc"][1]
        # DC only: colour = C0 * c0 + 0.5, exact to 1e-5 (test_sh.cpp:16-38)
        out = evaluate("dc")
        assert np.allclose(out[0], C0 * sh[0, :, 0] + 0.5, atol=1e-5)
        # degree 0 is direction independent (:40-58)
        assert np.array_equal(evaluate("dc_x"), out)
        # Y_1^-1 is antisymmetric in y (:60-84)
        up, dn = evaluate("y1_up"), evaluate("y1_down")
        assert np.allclose(up - 0.5, -(dn - 0.5), atol=1e-6)
        # degree 3 with zero higher coefficients == degree 0 (:106-125)
        assert np.allclose(evaluate("deg3_dc_only"), out, atol=1e-6)
        # batch == per item (:86-104)
        full = evaluate("batch")
        for i in range(5):
            assert np.array_equal(evaluate(f"batch_item{i}")[0], full[i])


def test_reference_input_validation(ref):
    """test_sh.cpp:127-143: bad degree / too few coefficients throw c10::Error in the reference."""
    assert ref["validation_rc"].tolist() == [1, 1, 0]


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as ge
    orc = ge.load_oracle()
    if not orc.ref_sh_available():
        sys.exit("oracle/_ref/libref_sh.so is not built (make -C oracle ref)")
    np.savez_compressed(GOLDEN, **_record_all(orc.ref_evaluate_sh_cpu))
    print("wrote", GOLDEN)
