"""The host mathematics of the similarity transform (cugs_similarity_init, transform.py) and the references the GPU
tests compare against (tests/transform_ref.py), on the CPU: band matrices against an independent fp64 fit, the fp32
mirror against the exact fp64 transform, the Similarity and camera algebra, and the ORACLE's own render invariance on
the cases the GPU render test uses."""
import numpy as np
import pytest

import transform_ref as tr

ULP = 2.0 ** -23


def _abi(pkg, R, t=(0, 0, 0), s=1.0):
    return tr.abi_matrices(pkg.Similarity(s, R, t).to_abi())


ROTATIONS = [tr.random_rotation(k) for k in range(1, 7)]


@pytest.mark.parametrize("k", range(len(ROTATIONS)))
def test_band_matrices_match_the_independent_fit(pkg, k):
    R = ROTATIONS[k]
    got, want = _abi(pkg, R)["d"], tr.fit_sh_rotation(R)
    for g, w in zip(got, want):
        assert g.dtype == np.float32
        err = float(np.max(np.abs(g.astype(np.float64) - w)))
        print(f"band {g.shape[0]}: max |D - fit| = {err:.3e}")
        assert err <= ULP
    for a, b in zip(pkg.sh_rotation_matrices(R), got):
        assert np.array_equal(a, b)


def test_band_matrices_are_orthogonal_and_a_representation(pkg):
    R1, R2 = ROTATIONS[0], ROTATIONS[1]
    d1, d2, d12, dt = (_abi(pkg, R)["d"] for R in (R1, R2, R1 @ R2, R1.T))
    for a, b, ab, at in zip(d1, d2, d12, dt):
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        assert np.max(np.abs(a64 @ a64.T - np.eye(a.shape[0]))) <= 1e-6
        assert np.max(np.abs(a64 @ b64 - ab)) <= 1e-6
        assert np.max(np.abs(at.astype(np.float64) - a64.T)) <= ULP      # D(R^T) = D(R)^T, each rounded once


def test_quarter_turns_about_z_are_exact_signed_permutations(pkg):
    R = np.eye(3)
    for turn in range(4):
        R = tr.ROT_Z90 @ R
        f = _abi(pkg, R)
        for D in f["d"]:
            assert np.all((D == 0) | (np.abs(D) == 1))
            assert np.array_equal(np.abs(D).sum(axis=0), np.ones(D.shape[0])) and \
                np.array_equal(np.abs(D).sum(axis=1), np.ones(D.shape[0]))
        assert np.array_equal(f["m"], R.astype(np.float32))
    assert f["flags"] == 3                                                # four quarter turns: the identity


def test_identity_is_exact(pkg):
    f = _abi(pkg, np.eye(3))
    for D in f["d"]:
        assert np.array_equal(D, np.eye(D.shape[0], dtype=np.float32))
    assert np.array_equal(f["m"], np.eye(3, dtype=np.float32)) and np.array_equal(f["q"], [1, 0, 0, 0])
    assert not f["t"].any() and f["log_scale"] == 0.0 and f["flags"] == 3
    assert _abi(pkg, np.eye(3), s=2.0)["flags"] == 1 and _abi(pkg, ROTATIONS[0])["flags"] == 2
    assert _abi(pkg, ROTATIONS[0], s=0.5)["flags"] == 0


def test_quaternion_and_matrix_fields(pkg):
    for R in ROTATIONS:
        f = _abi(pkg, R, t=(1.5, -2.0, 0.1), s=2.5)
        assert np.array_equal(f["m"], (2.5 * R).astype(np.float32))
        assert np.array_equal(f["t"], np.array([1.5, -2.0, 0.1], np.float32))
        assert f["log_scale"] == np.float32(np.log(2.5))
        q = tr.quat_of_rotation64(R)
        assert f["q"][0] >= 0 and np.max(np.abs(f["q"].astype(np.float64) - q)) <= ULP


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_colour_is_invariant_in_fp64(pkg, degree):
    """sum_k c'_k Y_k(R d) = sum_k c_k Y_k(d) with c' = D c, D from the independent fit (what exact64 applies)."""
    c = (degree + 1) ** 2
    arrays = dict(tr.make_arrays(pkg, 50, coeffs=c))
    d = tr.fixed_directions(50)
    for R in ROTATIONS[:3]:
        out, _ = tr.exact64(arrays, 1.0, R, np.zeros(3))
        before = np.einsum("nck,nk->nc", arrays["sh_coeffs"].astype(np.float64), tr.sh_basis64(d)[:, :c])
        after = np.einsum("nck,nk->nc", out["sh_coeffs"], tr.sh_basis64(d @ R.T)[:, :c])
        assert np.max(np.abs(after - before)) <= 1e-12


@pytest.mark.parametrize("coeffs", [1, 4, 9, 16])
def test_mirror_is_within_its_bound_of_the_exact_transform(pkg, coeffs):
    arrays = tr.make_arrays(pkg, 500, coeffs=coeffs)
    worst = 0.0
    for name, sim in tr.similarity_cases(pkg):
        got = tr.mirror32(arrays, sim.to_abi())
        want, mag = tr.exact64(arrays, sim.scale, sim.rotation, sim.translation)
        for k in ("positions", "rotations", "sh_coeffs"):
            err = np.abs(got[k].astype(np.float64) - want[k])
            bound = tr.MIRROR_FACTOR * mag[k]
            assert np.all(err <= bound), (name, k)
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        f32 = np.float32
        assert np.array_equal(got["scales"], arrays["scales"] + f32(np.log(sim.scale)) if sim.scale != 1.0
                              else arrays["scales"])
        assert np.array_equal(got["opacities"], arrays["opacities"])
        assert np.array_equal(got["sh_coeffs"][:, :, 0], arrays["sh_coeffs"][:, :, 0])
    print(f"C = {coeffs}: worst mirror error / bound = {worst:.3f}")


def test_mirror_respects_the_mask(pkg):
    arrays = tr.make_arrays(pkg, 64)
    mask = np.arange(64) % 3 == 0
    sim = tr.similarity_cases(pkg)[4][1]
    full, part = tr.mirror32(arrays, sim.to_abi()), tr.mirror32(arrays, sim.to_abi(), mask)
    for k in tr.PARAMS:
        assert np.array_equal(part[k][mask], full[k][mask]) and np.array_equal(part[k][~mask], arrays[k][~mask])


def test_similarity_algebra(pkg):
    S = pkg.Similarity
    a, b = S(2.5, ROTATIONS[0], [1.0, 2.0, 3.0]), S(0.4, ROTATIONS[1], [-0.5, 0.25, 4.0])
    x = np.random.Generator(np.random.Philox(key=9)).standard_normal((20, 3))
    assert np.max(np.abs(a.inverse().apply_points(a.apply_points(x)) - x)) <= 1e-12
    assert np.max(np.abs(a.compose(b).apply_points(x) - a.apply_points(b.apply_points(x)))) <= 1e-12
    assert np.max(np.abs(a.compose(b).matrix() - a.matrix() @ b.matrix())) <= 1e-12
    assert np.max(np.abs(a.compose(a.inverse()).matrix() - np.eye(4))) <= 1e-12
    r = S.from_matrix(a.matrix())
    assert abs(r.scale - a.scale) <= 1e-12 and np.max(np.abs(r.rotation - a.rotation)) <= 1e-12
    assert np.max(np.abs(r.translation - a.translation)) <= 1e-12
    xh = np.concatenate([x, np.ones((20, 1))], axis=1)
    assert np.max(np.abs((xh @ a.matrix().T)[:, :3] - a.apply_points(x))) <= 1e-12
    assert S().is_pure_translation() and S(1.0, np.eye(3), [1, 2, 3]).is_pure_translation()
    assert not a.is_pure_translation() and not S(2.0).is_pure_translation()
    with pytest.raises(ValueError):
        S.from_matrix(np.diag([1.0, 1.0, -1.0, 1.0]))
    with pytest.raises(ValueError):
        S(1.0, np.diag([1.0, 1.0, -1.0])).to_abi()


def test_transform_camera_is_the_matrix_product(pkg):
    sim = pkg.Similarity(2.5, ROTATIONS[2], [0.5, -1.0, 2.0])
    for view in (0, 3):
        cam = pkg.scene.make_camera(64, 48, view)
        new = pkg.transform_camera(cam, sim)
        assert new is not cam and new.rotation.dtype == np.float32 and new.translation.dtype == np.float32
        assert (new.width, new.height, new.intrinsics.fx) == (cam.width, cam.height, cam.intrinsics.fx)
        # view' = diag(s, s, s, 1) view inverse(sim): view' (sim x) = s (view x)
        V = np.eye(4)
        V[:3, :3], V[:3, 3] = cam.rotation.astype(np.float64), cam.translation.astype(np.float64)
        want = np.diag([sim.scale] * 3 + [1.0]) @ V @ np.linalg.inv(sim.matrix())
        assert np.max(np.abs(new.rotation - want[:3, :3] / 1.0)) <= 2.0 ** -23
        assert np.max(np.abs(new.translation - want[:3, 3])) <= 2.0 ** -23 * max(1.0, np.max(np.abs(want[:3, 3])))
    assert [c.translation.tolist() for c in pkg.transform_cameras([cam, cam], sim)] == [new.translation.tolist()] * 2


@pytest.mark.parametrize("up", [(0.0, 0.0, 1.0), (0.0, -1.0, 0.0), None])
def test_similarity_from_cameras(pkg, up):
    cams = [pkg.scene.make_camera(64, 48, v) for v in range(0, 12)]
    cams = pkg.transform_cameras(cams, pkg.Similarity(3.0, ROTATIONS[3], [5.0, -7.0, 2.0]))   # an arbitrary gauge
    sim = pkg.similarity_from_cameras(cams, radius=2.0, up=up)
    assert pkg.similarity_from_cameras(cams, radius=2.0, up=up).matrix().tolist() == sim.matrix().tolist()
    centres = np.stack([-(c.rotation.astype(np.float64).T @ c.translation.astype(np.float64)) for c in cams])
    moved = sim.apply_points(centres)
    assert np.max(np.abs(moved.mean(axis=0))) <= 1e-12
    assert abs(np.max(np.linalg.norm(moved, axis=1)) - 2.0) <= 1e-12
    ups = np.stack([-c.rotation.astype(np.float64)[1] for c in cams]).mean(axis=0)
    if up is None:
        assert np.array_equal(sim.rotation, np.eye(3))
    else:
        got = sim.rotation @ (ups / np.linalg.norm(ups))
        assert np.max(np.abs(got - np.asarray(up))) <= 1e-12
        assert abs(np.linalg.det(sim.rotation) - 1.0) <= 1e-12


def test_oracle_render_is_invariant_on_the_gpu_cases(pkg, orc):
    """The reference of tests/test_gpu_transform.py's render test: the oracle on (model, camera) and on the fp64-moved,
    once-rounded model with the moved camera.  No Gaussian changes radii > 0; the image moves by at most 2e-5."""
    for name, arrays, cam, sim, degree in tr.render_cases(pkg):
        depth = arrays["positions"][:, 2].min() * min(1.0, sim.scale)
        assert depth >= 0.8                                               # clear of the projection's cull at 0.2
        gap = tr.oracle_gap(orc, arrays, cam, sim, pkg, degree)
        print(f"{name}: oracle gap colour {gap['color']:.2e} alpha {gap['alpha']:.2e} depth {gap['depth']:.2e}")
        assert gap["same_visibility"], name
        assert gap["color"] <= 2e-5 and gap["alpha"] <= 2e-5 and gap["depth"] <= 2e-5, name
        assert int((gap["ref"]["radii"] > 0).sum()) > 0.5 * arrays["positions"].shape[0]
