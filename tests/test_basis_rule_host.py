"""No GPU: the rule that says whether the preconditioner's eigenbasis is stale (online_gp_amd/models/step_pacing.py), on hand-made
marginals.  Expected values are worked out from the rule's statement: a profile is a dimension's marginal over its max, clipped
below at 1e-2; the norm is the product of the profiles' sums; "moved" is a largest change beyond settings.precond_profile_drift; "slow"
is 2 more iterations than when the basis was fresh, with more than 1.1 times the mass."""
import numpy as np

from online_gp_amd import settings
from online_gp_amd.models.step_pacing import basis_kept, basis_slow, density_profiles, profiles_moved


def test_profiles_divide_by_the_max_and_clip_at_one_percent():
    margs = np.array([[2.0, 4.0, 0.0, 1.0],              # g = 4, holds a zero cell
                      [8.0, 0.04, 8.0, 0.0]])            # g = 3 (the last entry is padding): 0.04 / 8 = 0.005 < 1e-2
    profiles, norm = density_profiles(margs, (4, 3), 12)
    assert [p.tolist() for p in profiles] == [[0.5, 1.0, 1e-2, 0.25], [1.0, 1e-2, 1.0]]
    assert norm == (0.5 + 1.0 + 1e-2 + 0.25) * (1.0 + 1e-2 + 1.0)
    margs[:] = 0.0
    assert density_profiles(margs, (4, 3), 12) == (None, 12.0)
    one = density_profiles(np.array([[3.0, 3.0, 3.0]]), (3,), 3)        # one dimension
    assert one[0][0].tolist() == [1.0, 1.0, 1.0] and one[1] == 3.0


def test_moved_is_strictly_beyond_the_drift():
    drift = settings.precond_profile_drift.value()
    old = [np.array([1.0, 0.5]), np.array([0.0, 1.0, 1.0])]
    at = [old[0].copy(), np.array([drift, 1.0, 1.0])]                    # |drift - 0| is drift exactly
    above = [old[0].copy(), np.array([np.nextafter(drift, 1.0), 1.0, 1.0])]
    assert not profiles_moved(old, old)
    assert not profiles_moved(at, old)
    assert profiles_moved(above, old)
    assert profiles_moved([np.array([1.0, 0.25]), old[1]], old)          # any dimension, either sign: 0.25 > the default 0.2
    assert not profiles_moved([np.array([1.0, 0.375]), old[1]], old)
    with settings.precond_profile_drift(0.5):
        assert not profiles_moved(above, old)
        assert profiles_moved([old[0], np.array([0.75, 1.0, 1.0])], old)
    assert profiles_moved([np.array([np.nan, 0.5]), old[1]], old)        # not a number: re-solve
    assert profiles_moved([old[0], np.array([0.0, np.nan, 1.0])], old)


def test_slow_basis_notes_the_fresh_level_once_and_needs_more_mass():
    st = {"wsum": 100.0, "it0": None}
    assert not basis_slow(st, 0, 1000.0) and st["it0"] is None           # no solve yet: nothing to note
    assert not basis_slow(st, 3, 1000.0) and st["it0"] == 3              # the fresh level
    assert not basis_slow(st, 4, 1000.0) and st["it0"] == 3              # one more iteration: not yet; noted once
    assert basis_slow(st, 5, 1000.0) and st["it0"] == 3                  # it0 + 2 with more mass
    assert basis_slow(st, 7, np.nextafter(1.1 * 100.0, 200.0))
    assert not basis_slow(st, 5, 1.1 * 100.0)                            # exactly 1.1 times the mass is not more
    assert not basis_slow(st, 5, 100.0)
    basis_kept(st, 150.0)                                                # kept at a new scale: re-armed
    assert st == {"wsum": 150.0, "it0": None}
    assert not basis_slow(st, 5, 1000.0) and st["it0"] == 5              # 5 is the fresh level now
    assert not basis_slow(st, 6, 1000.0)
    assert not basis_slow(st, 7, 1.1 * 150.0) and basis_slow(st, 7, 166.0)
    assert not basis_slow({"wsum": 1.0}, 0, 2.0)                         # a state that never held the key
