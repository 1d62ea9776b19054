"""Host-side pacing of the streaming step (FixedNoiseOnlineSKIGP): where a warm refresh polls convergence first and when its carried
residual is recomputed (PollPacing), and the rule that says whether the preconditioner's eigenbasis is stale (density_profiles,
profiles_moved, basis_slow).  Pure host arithmetic: no device work, nothing of the model."""
from .. import settings


class PollPacing:
    """Poll placement and refresh pacing of one model's mean solve.  A model creates one in its constructor, so siblings and
    fantasies start with fresh pacing state."""

    __slots__ = ("default_tol", "hint", "sticky", "probe_pending", "probe_wait", "probe_gap", "probe_informed", "last_rel", "refreshes",
                 "queued")

    def __init__(self, default_tol):
        self.default_tol = default_tol       # of the residual that makes a probe "informed", where settings.cg_tolerance names none
        self.hint = 0                        # first poll of the next refresh, set after a cold solve
        self.sticky = 0                      # refreshes that still poll after 2 iterations: a new two-level block went in
        self.probe_pending = 0               # where the probe polled whose verdict is not in yet (deferred refreshes)
        self.probe_wait = 0                  # refreshes until the next probe
        self.probe_gap = 0                   # the wait after the last failed uninformed probe: 8, 16, 32
        self.probe_informed = False          # was the last probe invited by a small converged residual?
        self.last_rel = None                 # converged relative residual of the last solve (None: not kept)
        self.refreshes = 0                   # warm refreshes counted, for the every-16th residual recompute
        self.queued = (0, False)             # (first_check, probe) of the solve in flight (deferred refreshes)

    def place(self, last, auto=None):
        """Where a warm refresh polls convergence first: (iteration count, is this a probe?).  Streaming steps are alike (at
        50^3 the uniform bench stream needs 3 iterations for its first ~40 steps and 2 ever after; the clustered one 6, now and
        then 5), so the first poll goes where the previous refresh converged (`last`).  A *probe* polls one iteration earlier to notice
        that the stream got easier; one that fails costs a stand-alone vector update + poll and a host round trip (~14 us of a
        ~215 us step), one that is not made when it would have succeeded costs an iteration (41 us) per step.  So: probe
        every 4th refresh while the last converged residual says one iteration less might do (it is below tol / 10; the
        contraction per iteration is ~0.08 here: the residual after 3 iterations falls from 8e-5 to 7e-6 before 2 suffice),
        otherwise after 8, 16, 32 refreshes.  (Probing every other refresh, as before: 50 % failed polls, 0.221 ms per step
        against 0.216 with this placement, tools/policy_probe.py.)
        `auto` (not None: the step carries a deferred-poll handle and ``settings.poll_hindsight`` is on; its value says whether a
        solve is pending): -1, "place it by the hindsight of the previous solve" (include/wiski.h, first_check = -1) wherever the
        rules above would have answered from the history -- every poll reports where its solve first met the tolerance, so there is
        nothing to probe for.  Only the explicit hint of the first step after a cold solve stays."""
        if not last:
            return 0, False
        if auto is not None:
            self.sticky = self.probe_pending = 0
            return (min(last, self.hint) if self.hint and not auto else -1), False
        if self.sticky:
            # a new block of the two-level preconditioner went in: for this step and the next (whose `last` still predates the
            # switch: deferred refreshes report one step late) poll after 2 iterations, then after every one
            self.sticky -= 1
            return min(last, 2), False
        if self.hint:
            # the previous solve was a cold one: its count (8 at 50^3) says nothing about a warm, residual-carrying refresh
            # (3 there).  Poll early and then after every iteration -- a few extra polls instead of walking down from the
            # cold count one wasted iteration per refresh.
            return min(last, self.hint), False
        pend = self.probe_pending
        if pend:
            # deferred refreshes: the verdict of the probe queued by the previous step is not in yet (and `last` is older
            # still).  Poll where the probe did: if it fails this costs one more cheap poll, if it succeeds an iteration less.
            self.probe_pending = 0
            return pend, False
        wait = self.probe_wait
        rel = self.last_rel
        informed = rel is not None and rel < 0.1 * (settings.cg_tolerance.value() or self.default_tol)
        if informed:
            wait = min(wait, 4)
        probe = wait <= 0 and last > 1
        self.probe_informed = informed
        self.probe_wait = wait - 1
        fc = max(1, last - (1 if probe else 0))
        if probe:
            self.probe_pending = fc
        return fc, probe

    def verdict(self, it, fc, probe):
        """The solve polled first at `fc` took `it` iterations: what a probe has learnt."""
        if probe:
            self.probe_pending = 0
            if it <= fc:
                self.probe_gap, self.probe_wait = 0, 8          # cut to 4 by place() if the new residual invites it
            elif self.probe_informed:
                self.probe_wait = 4
            else:
                self.probe_gap = self.probe_wait = min(32, max(8, 2 * self.probe_gap))

    def solved(self, it, rel, fc, probe=False):
        """After a solve placed at (fc, probe): `it` iterations to the relative residual `rel` (None: the solve keeps none, probes
        are paced by the timer alone).  fc = -1: the library placed the poll, nothing to learn here."""
        if fc > 0:
            self.verdict(it, fc, probe)
        self.last_rel = rel

    def cold(self):
        """The solve just made was a cold one: the next refresh polls after 2 iterations (see place)."""
        self.hint = 2

    def warm(self):
        self.hint = 0

    def new_block(self):
        """A new block of the two-level preconditioner went in: the iteration count of the previous solves says little about the
        next one -- poll after 2 iterations, then after every one (the placement would otherwise walk down one iteration per probe)."""
        self.sticky = 2

    def queue(self, fc, probe):
        self.queued = (fc, probe)

    def count(self):
        self.refreshes += 1

    def uncount(self):
        """The refresh counted last was never queued."""
        self.refreshes -= 1

    def recompute_due(self):
        """Every 16th refresh recomputes the carried residual R = b - Z - A U from scratch, so that the fp rounding of its recursion
        cannot accumulate."""
        return self.refreshes % 16 == 0


def density_profiles(margs, g, m):
    """(profiles, norm) of the preconditioner's density model from the host marginals [d, max g] of the row sums of W^T D^-1 W (rows
    padded with zeros, none negative): per dim the marginal over its g[q] nodes divided by its maximum and clipped below at 1e-2;
    norm = prod_q sum(profile_q).  No positive mass: (None, m), the constant model."""
    if not margs.max() > 0:
        return None, float(m)
    profiles, norm = [], 1.0
    for q, gq in enumerate(g):
        t = (margs[q, :gq] / margs[q, :gq].max()).clip(1e-2, None)
        profiles.append(t)
        norm *= float(t.sum())
    return profiles, norm


def profiles_moved(profiles, old):
    """Has the normalised density profile left the one the eigenbasis was solved for: is its largest change over all dims beyond
    settings.precond_profile_drift?  (A change that is not a number counts as moved: the basis is re-solved.)"""
    drift = settings.precond_profile_drift.value()
    return not all(float(abs(a - b).max()) <= drift for a, b in zip(profiles, old))


def basis_slow(st, its, wsum):
    """The symptom of a stale eigenbasis: the refresh needs 2 more iterations than the first one after the basis `st` was solved (or
    kept at a new scale: basis_kept) did, and the mass has grown by 10 % since.  Notes that first count in st["it0"]."""
    if st.get("it0") is None and its > 0:
        st["it0"] = its                                  # iteration level of this basis when it was fresh
    return st.get("it0") is not None and its >= st["it0"] + 2 and wsum > 1.1 * st["wsum"]


def basis_kept(st, wsum):
    """Same density shape at the mass `wsum`: the eigenbasis stays, only the scale moves; basis_slow starts over."""
    st["wsum"] = wsum
    st["it0"] = None
