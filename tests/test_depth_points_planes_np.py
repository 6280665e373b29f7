"""The plane fit's restatement (depth_points_planes_np.py; include/dmi.h: dmi_fit_point_planes) on cases worked out by
hand: points on a plane keep their bits and get the plane's normal on the old normal's side, a lifted point moves by the computed
step, the tie at the radius is a member, coincident points get the procedure's normal, min_neighbors and the flags, and a noisy
sphere cap comes closer to its sphere.  No GPU."""
import numpy as np
import pytest

import depth_points_planes_np as F


def _plane(z=0.5):
    xy = np.array([[i, j] for i in range(5) for j in range(5)], dtype=np.float64) * 0.125      # lattice-friendly: radius 0.25 has s = 2^16
    return np.concatenate([xy, np.full((25, 1), z)], axis=1)


def test_points_on_a_plane_keep_their_bits_and_get_its_normal():
    xyz = _plane()
    up = np.tile(np.array([[0.0, 0.6, 0.8]], dtype=np.float32), (25, 1))
    for old, side in ((up, 1.0), (-up, -1.0), (None, 1.0)):
        out, report = F.fit_planes(xyz, old, 0.25, 3, 3)
        assert out["xyz"].tobytes() == xyz.tobytes() and report["fitted"] == 25 and report["max_shift"] == 0.0
        assert np.all(out["normal"] == np.array([0.0, 0.0, side], dtype=np.float32)) and np.all(out["plane_rms"] == 0.0)
    assert F.lattice(0.25) == (65536.0, 1.0 / 65536.0) and F.lattice(0.1) == (2.0 ** 18, 2.0 ** -18)


def test_a_lifted_point_moves_by_the_computed_step():
    xyz = _plane(0.0)
    xyz[12, 2] = 1.0 / 64                                              # the centre, lifted by 1024 lattice units
    out, report = F.fit_planes(xyz, None, 0.1875, 3, 1)
    m, S, T = F.moments(xyz, 0.1875)
    assert m[12] == 9 and S[12].tolist() == [0, 0, -8 * 2048]          # s = 2^17: its eight neighbours lie 2048 units below it
    t, n, rms = F.results_from_moments(m[12:13], S[12:13], T[12:13], 2.0 ** -17, np.zeros((1, 3)))
    assert abs(n[0, 2]) == 1.0 and abs(t[0]) == (8 * 2048 / 9) * 2.0 ** -17
    assert out["xyz"][12, 2] == xyz[12, 2] + t[0] * n[0, 2] and 0 < out["xyz"][12, 2] < xyz[12, 2]
    assert out["normal"].tobytes() == np.zeros((25, 3), dtype=np.float32).tobytes()            # MOVE alone: the normals keep their bits
    assert report["max_shift"] >= abs(t[0])


def test_the_tie_at_the_radius_is_a_member():
    for s in (1.0, 2.0 ** -20, 2.0 ** 30):
        tie = np.array([[0.0, 0.0, 0.0], [3 * s, 4 * s, 0.0], [1.5 * s, 2 * s, s]])
        m, S, _ = F.moments(tie, 5 * s)
        assert m.tolist() == [3, 3, 3]
        scale, _ = F.lattice(5 * s)                                   # 5 s = 0.625 * 2^3 s
        assert S[0].tolist() == [int(4.5 * s * scale), int(6 * s * scale), int(s * scale)]
        assert F.moments(tie, np.nextafter(5 * s, 0.0))[0].tolist() == [2, 2, 3]


def test_coincident_points_get_the_procedures_normal():
    same = np.tile(np.array([[3.25, -1.5, 2.0]]), (6, 1))
    out, report = F.fit_planes(same, None, 1e-3, 2, 3)
    assert report["fitted"] == 6 and np.all(out["normal"] == [1.0, 0.0, 0.0]) and np.all(out["plane_rms"] == 0.0)
    assert out["xyz"].tobytes() == same.tobytes()
    old = np.tile(np.array([[-1.0, 0.0, 0.0]], dtype=np.float32), (6, 1))
    assert np.all(F.fit_planes(same, old, 1e-3, 2, 2)[0]["normal"] == [-1.0, 0.0, 0.0])


def test_min_neighbors_and_the_flags():
    rng = np.random.default_rng(4)
    xyz = np.concatenate([_plane() + rng.normal(scale=0.004, size=(25, 3)), [[9.0, 9.0, 9.0], [9.0, 9.0625, 9.0]]])
    old = np.tile(np.array([[0.0, 0.0, -1.0]], dtype=np.float32), (27, 1))
    both, report = F.fit_planes(xyz, old, 0.25, 3, 3)
    assert report["fitted"] == 25 and report["unsupported"] == 2 and report["crowded"] == 0
    assert both["plane_rms"][25:].tolist() == [-1.0, -1.0] and np.all(both["plane_rms"][:25] > 0)
    assert both["xyz"][25:].tobytes() == xyz[25:].tobytes() and both["normal"][25:].tobytes() == old[25:].tobytes()
    assert both["neighbors"][25:].tolist() == [1, 1] and np.all(both["normal"][:25, 2] < -0.9)
    moved, _ = F.fit_planes(xyz, old, 0.25, 3, F.MOVE)
    turned, turned_report = F.fit_planes(xyz, old, 0.25, 3, F.NORMALS)
    assert moved["xyz"].tobytes() == both["xyz"].tobytes() and moved["normal"].tobytes() == old.tobytes()
    assert turned["normal"].tobytes() == both["normal"].tobytes() and turned["xyz"].tobytes() == xyz.tobytes() and turned_report["max_shift"] == 0.0
    assert F.fit_planes(xyz, old, 0.25, 24, 3)[1]["fitted"] < 25
    for bad in (dict(min_neighbors=1, flags=3), dict(min_neighbors=3, flags=0), dict(min_neighbors=3, flags=4)):
        with pytest.raises(ValueError):
            F.fit_planes(xyz, old, 0.25, **bad)
    for radius in (0.0, -1.0, float("nan"), float("inf"), 1e-200, 1e200):
        with pytest.raises(ValueError):
            F.fit_planes(xyz, old, radius, 3, 3)


def test_a_noisy_sphere_cap_comes_closer_to_its_sphere():
    rng = np.random.default_rng(1)
    u = rng.normal(size=(800, 3))
    u[:, 2] = np.abs(u[:, 2]) + 2
    u /= np.linalg.norm(u, axis=1)[:, None]
    xyz = u * (1 + rng.normal(scale=0.004, size=(800, 1)))
    out, report = F.fit_planes(xyz, u.astype(np.float32), 0.1, 5, 3)
    fit = out["plane_rms"] >= 0
    before = np.sqrt(np.mean((np.linalg.norm(xyz[fit], axis=1) - 1) ** 2))
    after = np.sqrt(np.mean((np.linalg.norm(out["xyz"][fit], axis=1) - 1) ** 2))
    print("RMS distance to the sphere: %.5f before, %.5f after, %d of %d fitted" % (before, after, report["fitted"], report["points_in"]))
    assert report["fitted"] > 600 and after < before
