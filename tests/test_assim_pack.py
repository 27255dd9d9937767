"""The host-side helpers of the assimilation, without the library: _pack.pack_observations (the arrays fs_batch_assimilate takes) and
flowsim_amd.assimilation (the Gaspari-Cohn taper, the seeded observation perturbations, the cycle's bookkeeping)."""
import numpy as np
import pytest

from flowsim_amd import _abi as A
from flowsim_amd import _pack as P
from flowsim_amd import assimilation as DA


def test_pack_observations_builds_the_arrays_of_the_call():
    obs = [DA.Observation(2, "stage", 412.5, 0.01), (0, "flow", 50, 4), (1, 3, 1.5, 0.25)]
    m, gauge, signal, value, variance, pert, taper, floor = P.pack_observations(obs, 5, 7)
    assert m == 3 and pert is None and taper is None and floor == 1e-3
    assert gauge.dtype == signal.dtype == np.int32 and value.dtype == variance.dtype == np.float64
    assert gauge.tolist() == [2, 0, 1] and signal.tolist() == [2, 1, 3] and value.tolist() == [412.5, 50.0, 1.5] and variance.tolist() == [0.01, 4.0, 0.25]
    e = np.arange(15.0).reshape(3, 5)
    _, _, _, _, _, pert, taper, floor = P.pack_observations(obs, 5, 7, perturbations=e[:, ::1], taper=np.linspace(0, 1, 7), depth_floor=0)
    assert pert.flags.c_contiguous and np.array_equal(pert, e) and floor == 0.0
    assert taper.shape == (3, 7) and taper.flags.c_contiguous and np.array_equal(taper[2], np.linspace(0, 1, 7))
    both = np.random.default_rng(0).uniform(0, 1, (3, 7))
    assert np.array_equal(P.pack_observations(obs, 5, 7, taper=both)[6], both)
    assert P.pack_observations(obs, 5, 7, perturbations=np.asfortranarray(e))[5].flags.c_contiguous


def test_pack_observations_refuses_what_has_no_shape():
    obs = [(0, "stage", 1.0, 1.0)]
    with pytest.raises(ValueError, match="1 .. 16 observations"):
        P.pack_observations([], 5, 7)
    with pytest.raises(ValueError, match="1 .. 16 observations"):
        P.pack_observations(obs * (A.ASSIM_MAX_OBS + 1), 5, 7)
    assert P.pack_observations(obs * A.ASSIM_MAX_OBS, 5, 7)[0] == 16
    with pytest.raises(ValueError, match="gauge, signal, value, variance"):
        P.pack_observations([(0, "stage", 1.0)], 5, 7)
    with pytest.raises(ValueError, match="unknown gauge signal"):
        P.pack_observations([(0, "level", 1.0, 1.0)], 5, 7)
    with pytest.raises(ValueError, match="perturbations are"):
        P.pack_observations(obs, 5, 7, perturbations=np.zeros((5, 1)))
    with pytest.raises(ValueError, match="taper is"):
        P.pack_observations(obs, 5, 7, taper=np.zeros(5))
    assert A.ASSIM_CHUNK == 256 and "fs_batch_assimilate" in A.SIGNATURES


def test_gaspari_cohn_is_one_at_zero_and_gone_from_twice_the_radius():
    c = 2500.0
    assert DA.gaspari_cohn(0.0, c) == 1.0 and DA.gaspari_cohn(-0.0, c) == 1.0
    x = np.linspace(0.0, 3.0 * c, 3001)
    g = DA.gaspari_cohn(x, c)
    assert np.all(g[x >= 2.0 * c] == 0.0) and g[x < 2.0 * c].min() > 0.0 and np.all((g >= 0.0) & (g <= 1.0))
    assert np.all(np.diff(g) <= 0.0) and np.all(np.diff(g[x < 2.0 * c]) < 0.0)       # monotone, strictly inside the support
    assert np.array_equal(DA.gaspari_cohn(-x, c), g)                                 # even
    # continuous at the radius, where the two polynomials meet (5 / 24), and at twice the radius, where the second one ends
    at = lambda z: float(DA.gaspari_cohn(z * c, c))
    assert abs(at(1.0) - 5.0 / 24.0) <= 4e-16 and abs(at(np.nextafter(1.0, 2.0)) - at(1.0)) <= 1e-15
    assert at(np.nextafter(2.0, 0.0)) <= 1e-15
    assert np.max(np.abs(np.diff(g))) <= 1.2 * (x[1] / c)                            # no jump anywhere: the slope is at most ~1 / radius
    with pytest.raises(ValueError):
        DA.gaspari_cohn(1.0, 0.0)
    t = DA.taper(np.arange(7) * 1000.0, [0.0, 2250.0], c)
    assert t.shape == (2, 7) and t[0, 0] == 1.0 and t[0, 5] == 0.0 and t[1, 2] > t[1, 3] > t[1, 1] > 0.0


def test_perturbations_are_the_seeds_and_centred_over_the_active_members():
    var = np.array([0.01, 4.0, 0.25])
    a, b = DA.perturbations(7, var, 200), DA.perturbations(7, var, 200)
    assert a.shape == (3, 200) and a.flags.c_contiguous and a.tobytes() == b.tobytes()       # same seed, same bits
    assert DA.perturbations(8, var, 200).tobytes() != a.tobytes()
    assert np.all(np.abs(a.std(axis=1, ddof=1) / np.sqrt(var) - 1.0) < 0.2)                  # N(0, variance): 200 draws, 4 sigma of the estimate
    active = np.ones(200, dtype=bool); active[[4, 77, 199]] = False
    c = DA.perturbations(7, var, 200, active=active)
    assert np.all(c[:, ~active] == 0.0)
    for j in range(3):                                                                       # zero mean to rounding: n eps of the sum of magnitudes
        assert abs(c[j, active].sum()) <= 200 * 2.0 ** -52 * np.abs(c[j]).sum()
    assert np.allclose(c[:, active], a[:, active] - a[:, active].mean(axis=1, keepdims=True), rtol=0, atol=1e-15)
    assert np.all(DA.perturbations(1, [0.0], 5) == 0.0)
    with pytest.raises(ValueError):
        DA.perturbations(1, [-1.0], 5)
    with pytest.raises(ValueError):
        DA.perturbations(1, [1.0], 5, active=np.zeros(5, dtype=bool))


class _FakeBatch:
    """what cycle() touches of a PreissmannBatch"""
    def __init__(self):
        self.level, self.calls = 0, []

    def step(self, n):
        self.level += n
        self.calls.append(("step", n))

    def assimilate(self, observations, perturbations, taper, depth_floor):
        self.calls.append(("assimilate", self.level, observations, perturbations, taper, depth_floor))
        return dict(n_active=3)


def test_cycle_steps_to_each_observation_level_and_assimilates_there():
    b = _FakeBatch()
    obs = [DA.Observation(0, "stage", 1.0, 1.0)]
    out = list(DA.cycle(b, [(5, obs, None, None), (5, obs, "e", "t"), (12, obs, None, None)], depth_floor=0.5))
    assert [k for k, _ in out] == [5, 5, 12] and all(d == dict(n_active=3) for _, d in out)
    assert b.calls == [("step", 5), ("assimilate", 5, obs, None, None, 0.5), ("assimilate", 5, obs, "e", "t", 0.5), ("step", 7),
                       ("assimilate", 12, obs, None, None, 0.5)]
    with pytest.raises(ValueError, match="behind the batch"):
        list(DA.cycle(b, [(3, obs, None, None)]))
