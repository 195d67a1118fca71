"""tests/list_check_ref.py on hand-made cases (no GPU): the reference of tests/test_gpu_list_checks.py must itself take the nearest image and find the
right atom, or every device comparison built on it is void."""
import numpy as np

from tests import list_check_ref as R


def test_two_atoms_across_a_face():
    """atom 0 flew 0.03 nm through the +x face of a 3 nm box and was wrapped; atom 1 moved 0.004 nm inside: d² is 0.03², not (3 − 0.03)²"""
    L = 3.0
    Q = np.array([[2.99, 1.0, 1.0], [1.0, 1.0, 1.0]])
    X = np.array([[0.02, 1.0, 1.0], [1.0, 1.004, 1.0]])
    d2 = R.disp2(X, Q, L)
    assert np.allclose(d2, [0.03 ** 2, 0.004 ** 2], rtol=1e-12, atol=0)
    i, top, nxt = R.top_two(d2)
    assert i == 0 and np.isclose(np.sqrt(top), 0.03) and np.isclose(np.sqrt(nxt), 0.004)
    # per axis: a box that is periodic-long in y keeps a y move as it is
    assert np.allclose(R.disp2([[0.0, 0.02, 0.0]], [[0.0, 4.99, 0.0]], [3.0, 5.0, 3.0]), [0.03 ** 2])
    assert np.allclose(R.disp2([[0.0, 2.5, 0.0]], [[0.0, 0.5, 0.0]], [3.0, 5.0, 3.0]), [4.0])


def test_sheared_cell():
    """a cell sheared in xy and xz; an atom that leaves through the sheared b-face comes back displaced by −b, which has an x component: the per-axis
    image of a cubic box would be wrong by that shear, the fractional one is not"""
    B = np.array([[3.0, 0.0, 0.0], [0.9, 2.8, 0.0], [0.5, 0.4, 2.6]])
    step = np.array([0.01, 0.025, -0.005])
    q = 0.3 * B[0] + 0.999 * B[1] + 0.4 * B[2]                 # just inside the +b face
    x = q + step - B[1]                                        # flew through it, wrapped by −b
    d2 = R.disp2([x], [q], np.diag(B), basis=B)
    assert np.allclose(d2, [step @ step], rtol=1e-10, atol=0)
    wrong = R.disp2([x], [q], np.diag(B))                      # what a per-axis image would report
    assert wrong[0] > 100 * d2[0]
    # through the c-face as well, both at once
    x2 = q + step - B[1] + B[2]
    assert np.allclose(R.disp2([x2], [q], np.diag(B), basis=B), [step @ step], rtol=1e-10, atol=0)
    # a cubic basis agrees with the per-axis form
    rng = np.random.default_rng(3)
    Q = rng.uniform(0, 3, (50, 3)); X = Q + rng.normal(scale=0.02, size=(50, 3))
    X -= np.floor(X / 3.0) * 3.0
    assert np.allclose(R.disp2(X, Q, 3.0), R.disp2(X, Q, 3.0, basis=np.eye(3) * 3.0), rtol=1e-9, atol=1e-18)


def test_speed_over_owned_atoms_only():
    V = np.array([[0.1, 0.0, 0.0], [0.0, -0.3, 0.4], [2.0, -1.0, 0.5]])
    assert np.isclose(R.speed2(V).max(), 5.25)
    assert np.isclose(R.speed2(V, n_owned=2).max(), 0.25)


def test_tolerances_are_far_below_an_omitted_runner():
    """an omitted runner is a factor >= 4 in d² and v²; the arithmetic bounds are below 1e-3 relative in fp32 at the magnitudes of the tests"""
    for dt in (np.float32, np.float64):
        for d in (0.012, 0.03, 0.0455):
            assert R.tol_d2(dt, 30.0, d * d, triclinic=True) < 2e-2 * d * d
            assert R.tol_d2(dt, 3.3, d * d) < 1e-3 * d * d
        assert R.tol_v2(dt, 5.25) < 1e-6 * 5.25
    assert R.tol_d2(np.float64, 3.3, 9e-4) < 1.3e-7 * 9e-4      # fp64: the one cast to float is all that is left
