"""No GPU: the host's poll-placement and refresh-pacing policy (online_gp_amd/models/step_pacing.py: PollPacing) replayed through
scripted histories and compared, answer for answer, with what the model's own placement methods answered before the policy moved
into the class (tests/golden/poll_placement_trace.json, recorded at the parent of the commit that added this file; the adapter that
recorded it is in that commit's message).  Integers and booleans: no tolerance."""
import json
import os

from online_gp_amd import settings

TRACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poll_placement_trace.json")


def scenarios():
    """Each streams `need[t]` (the iterations step t needs) after a cold solve that took 8.  rel: the converged residual every solve
    reports (None: the generic refresh, which keeps none).  deferred: the result of step t is noted after the placement of step
    t + 1.  auto_from: from that step on the placement is asked with auto = "a solve is queued"."""
    road = [3] * 60 + [2] * 80
    return [
        dict(name="stream_new_block", dtype="float32", need=[3] * 30 + [2] * 30 + [6] * 20 + [5] * 60, rel=5e-9, new_block_at=50),
        dict(name="uninformed_gap_8_16_32", dtype="float32", need=road, rel=5e-8),
        dict(name="generic_refresh", dtype="float64", need=[4] * 40 + [1] * 40, rel=None, generic=True),
        dict(name="deferred", dtype="float32", need=[3] * 30 + [2] * 30, rel=5e-9, deferred=True),
        dict(name="deferred_auto_from_5", dtype="float32", need=[3] * 10 + [2] * 10, rel=5e-9, deferred=True, auto_from=5),
        dict(name="fresh_object", dtype="float32", fresh=[0, 1]),
        dict(name="informed_under_cg_tolerance_1e-6", dtype="float32", need=road, rel=5e-8, cg_tolerance=1e-6),
        dict(name="refresh_counter", dtype="float32", refreshes=40, uncount_at=15),
        dict(name="deferred_auto_from_0", dtype="float32", need=[3] * 6, rel=5e-9, deferred=True, auto_from=0),
        dict(name="uninformed_gap_stays_32", dtype="float32", need=[3] * 140, rel=5e-8),
        dict(name="deferred_new_block", dtype="float32", need=[3] * 12 + [5] * 12, rel=5e-9, deferred=True, new_block_at=12),
    ]


def _run(a, sc):
    """Drive adapter `a` through scenario `sc`; every answer it gives, in order."""
    out = []
    if "fresh" in sc:
        return [list(a.place(last)) for last in sc["fresh"]]
    if "refreshes" in sc:
        out.append(a.recompute_due())                      # read before anything was counted
        for t in range(sc["refreshes"]):
            a.count()
            if t == sc["uncount_at"]:
                out.append(a.recompute_due())
                a.uncount()
            out.append(a.recompute_due())
        return out
    last, queued = 8, None
    a.cold()
    for t, need in enumerate(sc["need"]):
        if t == sc.get("new_block_at"):
            a.new_block()
        if sc.get("generic"):
            a.count()
        auto = (queued is not None) if sc.get("auto_from") is not None and t >= sc["auto_from"] else None
        fc, probe = a.place(last, auto)
        out.append([fc, probe])
        if sc.get("generic"):
            out.append(a.recompute_due())
        it = need if fc <= 0 else max(fc, need)            # the stand-in solve: polls at fc, then after every iteration
        if sc.get("generic"):
            a.refresh_done(it, fc, probe)
            a.warm()
            last = it
        elif sc.get("deferred"):
            if queued is not None:
                a.solve_done(*queued)
                last = queued[0]
            queued = (it, sc["rel"], fc, probe)
        else:
            a.solve_done(it, sc["rel"], fc, probe)
            last = it
    return out


def replay(adapter):
    """{scenario name: answers} of `adapter(dtype name)` objects, one per scenario."""
    res = {}
    for sc in scenarios():
        with settings.cg_tolerance(sc.get("cg_tolerance")):
            res[sc["name"]] = _run(adapter(sc["dtype"]), sc)
    return res


class _Adapter:
    """The operations of the replay on a PollPacing, composed as the model composes them."""

    def __init__(self, dtype):
        from online_gp_amd.models.step_pacing import PollPacing        # (here: scenarios() and replay() also import at the parent commit)

        self.p = PollPacing(1e-7 if dtype == "float32" else 1e-11)
        for name in ("place", "verdict", "new_block", "cold", "warm", "count", "uncount", "recompute_due"):
            setattr(self, name, getattr(self.p, name))

    def solve_done(self, it, rel, fc, probe):              # FixedNoiseOnlineSKIGP._note_solve
        self.p.solved(it, rel, fc, probe)
        self.p.warm()

    def refresh_done(self, it, fc, probe):                 # the generic refresh of prediction_cache: no residual kept
        self.p.solved(it, None, fc, probe)


def test_placement_and_pacing_answer_as_recorded():
    with open(TRACE) as f:
        want = json.load(f)
    got = replay(_Adapter)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


def test_the_scenarios_reach_what_they_are_there_for():
    """Read off the recorded trace, so that a scenario cannot quietly stop exercising its branch."""
    with open(TRACE) as f:
        want = json.load(f)
    probes = lambda name: [t for t, (fc, probe) in enumerate(want[name]) if probe]
    gaps = lambda name: [b - a for a, b in zip(probes(name), probes(name)[1:])]
    assert want["fresh_object"] == [[0, False], [1, False]]
    assert want["stream_new_block"][0] == [2, False]                       # the cold hint
    assert want["stream_new_block"][50] == want["stream_new_block"][51] == [2, False]     # the sticky hint of a new block
    g = gaps("uninformed_gap_8_16_32")
    assert g[:3] == [9, 17, 33] and max(g) == 33       # waits of 8, 16, 32 refreshes (and the probing one), capped at 32
    assert gaps("uninformed_gap_stays_32") == [9, 17, 33, 33, 33]
    assert set(gaps("informed_under_cg_tolerance_1e-6")) == {5}            # 5e-8 is informed there: a wait of 4
    assert [-1, False] in want["deferred_auto_from_5"] and want["deferred_auto_from_0"][0] == [2, False]
    assert want["refresh_counter"].count(True) == 4                        # at 0, 16, 16 again after the uncount, 32
    assert want["generic_refresh"][1] is False and True in want["generic_refresh"][1::2]
