"""The spawn rule bodies against the reference's own, unmodified rule methods (tests/golden/spawn_rule_bodies.npz, written by
``gen_golden.py rules``): the checker (oracle/fo_spawn_rules_ref.py) replays every recorded scene on the CPU and has to return
the reference's decisions -- the same ordered (agent type, source) list from ``find`` and from each family, positions and
curvilinear positions to 1e-9, orientations to 1e-12, the same cell.  Both sides share one discretisation (the geometry under
the rules is the build's), so no wider margin is justified; the tolerances are those of ``_same`` in
tests/test_spawn_rules_gpu.py.  The fixture also carries the lines of spawn_locator.py the recording executed: every executable
line of the rule bodies has to be among them, save the allow-list below."""
import numpy as np
import pytest

import spawn_rule_cases as SC

# spawn_locator.py: dynamic rule, static rule, turn rule, rectangle fit + metrics
RANGES = ((145, 317), (323, 476), (481, 578), (695, 726))
# executable lines of those ranges the recording may leave out, each with its reason
ALLOWED_UNHIT = {
    238: "debug: `pass` under `visualization is not None and debug`",
    262: "debug print (opposite direction)",
    268: "debug print (other direction)",
    313: "debug plot of the occluded area",
    314: "debug plot of the Car rectangle",
    315: "debug plot of the Bicycle rectangle",
    441: "a point on the boundary of the visible area buffered by 0.195 m is 0.195 m away from it: its 0.15 m disc cannot "
         "touch it (the candidate is the sample just outside the buffer)",
    471: "debug plot of the cross line",
    472: "debug plot of the spawn position",
    531: "debug print (MultiLineString)",
    533: "raise ValueError('Unknown intersection type!'): a line cut by an area is empty, one part or several",
}
LINE_MULTIPOINT, LINE_MULTILINESTRING = 421, 529     # first line of the MultiPoint branch / the MultiLineString assignment
MIN_CASES = 200
MAX_RAISING_SHARE = 0.10
MIN_CASES_WITH_POINTS = 30          # per family
MIN_BRANCH_CASES = 10               # MultiPoint, MultiLineString
FAMILY_OF_SOURCE = (("behind_dynamic_obstacle", "dynamic"), ("behind static obstacle", "static"), ("left turn", "turn"),
                    ("right turn", "turn"))


def _family(source):
    return next(f for prefix, f in FAMILY_OF_SOURCE if source.startswith(prefix))


def check_fixture(loaded):
    """the conditions the fixture has to meet, from the reference run alone: coverage, caps, minimum counts"""
    cases, z = loaded
    assert len(cases) >= MIN_CASES
    missed = sorted(set(z["lines_executable"].tolist()) - set(z["lines_hit"].tolist()))
    assert all(any(a <= n <= b for a, b in RANGES) for n in z["lines_executable"].tolist())
    assert [n for n in missed if n not in ALLOWED_UNHIT] == [], "lines of the rule bodies no recorded scene executes"
    raising = [k for k, (_, r) in enumerate(cases) if any(c[0] == SC.RAISES for c in r["calls"].values())]
    assert len(raising) <= MAX_RAISING_SHARE * len(cases), (len(raising), len(cases))
    with_points = {"dynamic": 0, "static": 0, "turn": 0}
    for _, r in cases:
        fams = {f for f in with_points if r["calls"][f][2]} | {_family(p[1]) for p in r["calls"]["find"][2]}
        for f in fams:
            with_points[f] += 1
    assert all(n >= MIN_CASES_WITH_POINTS for n in with_points.values()), with_points
    n_mp, n_ml = sum(r["multipoint"] for _, r in cases), sum(r["multiline"] for _, r in cases)
    assert n_mp >= MIN_BRANCH_CASES and n_ml >= MIN_BRANCH_CASES, (n_mp, n_ml)
    maxima = {(c.max_static, c.max_dynamic) for c, _ in cases}
    assert {m for pair in maxima for m in pair} >= {0, 1, 3}
    return dict(raising=len(raising), with_points=with_points, multipoint=n_mp, multilinestring=n_ml,
                frames=[sum(c.frame == f for c, _ in cases) for f in (0, 1)], missed=missed)


@pytest.fixture(scope="module")
def fixture():
    return SC.load_fixture()


def test_fixture_meets_its_conditions(fixture):
    stats = check_fixture(fixture)
    assert stats["frames"][1] >= 10          # a share of the cases runs through a caller's frame


def compare(recorded, got, view):
    """the recorded call against a list of SpawnPoint: None when they agree, else what differs"""
    status, _, want = recorded
    have = SC.points_of(list(got) if isinstance(got, list) else got)
    if [(p[0], p[1]) for p in want] != [(p[0], p[1]) for p in have]:
        return f"types/sources {[(p[0], p[1]) for p in have]} != reference {[(p[0], p[1]) for p in want]}"
    for a, b in zip(have, want):
        if view._cell(a[2]) != view._cell(b[2]):
            return f"cell {view._cell(a[2])} != {view._cell(b[2])}"
        if not np.abs(a[2] - b[2]).max() <= 1e-9:
            return f"position off by {np.abs(a[2] - b[2]).max():.3g}"
        if (a[3] is None) != (b[3] is None) or (a[3] is not None and not np.abs(a[3] - b[3]).max() <= 1e-9):
            return f"cl_pos {a[3]} != {b[3]}"
        if (a[4] is None) != (b[4] is None) or (a[4] is not None and not abs(a[4] - b[4]) <= 1e-12):
            return f"orientation {a[4]} != {b[4]}"
    return None


def checker_calls(oracle, case):
    """what the checker returns for the four recorded calls of a case, its intention and the view"""
    from oracle.fo_spawn_rules_ref import SpawnRules
    view, obs, lane_yaw_at, lanelet_of = SC.cpu_scene(oracle, case)
    cs = SC.frame_of(case)
    ego_cl = cs.convert_to_curvilinear_coords(case.ego[0], case.ego[1])
    rules = SpawnRules(case.cfg, case.path, cs, lane_yaw_at, lanelet_of, obs, lanelets=case.lanelets,
                       intersections=case.intersections)
    got = {"find": rules.find(view, case.ego, ego_cl, case.v, case.yaw)}
    got["dynamic"] = rules.behind_dynamic_obstacle(view)
    got["static"] = rules.behind_static_obstacle(view)
    got["turn"] = rules.behind_turn_point(view, rules.last_intention) if rules.last_intention != "straight ahead" else None
    return got, rules.last_intention, view


def continued(slot, got, case, view):
    """a call in which the reference raises: the project skips the obstacle, leaves a type out or gives no point instead
    (DESIGN.md section 6), so what it returns is still an answer of that rule -- no point where no turn is intended, else
    points of the slot's own family on road cells (a pedestrian behind a parked car on an unseen one), each parked car named once, no more than the rule's count check
    lets through (one obstacle beyond the maximum; a Car and a Bicycle per dynamic obstacle).  None when that holds."""
    if slot == "turn":
        return None if got is None or hasattr(got, "agent_type") and _family(got.source) == "turn" else f"turn gave {got}"
    if not isinstance(got, list):
        return f"no list but {got!r}"
    pts = SC.points_of(got)
    if slot != "find" and any(_family(p[1]) != slot for p in pts):
        return f"points of another family {[p[1] for p in pts]}"
    for p in pts:
        cls = int(view.class_at(p[2])) if np.isfinite(p[2]).all() else 0
        if not cls & 1 or (_family(p[1]) == "static" and cls & 2):     # (:440, :444: a pedestrian's disc is on the road, unseen)
            return f"{p[0]} at {p[2]} off the road or in sight"
    static = [p[1] for p in pts if _family(p[1]) == "static"]
    n_dynamic = sum(_family(p[1]) == "dynamic" for p in pts)
    if len(set(static)) != len(static) or len(static) > case.max_static + 1 or n_dynamic > 2 * (case.max_dynamic + 1):
        return f"too many points {[p[1] for p in pts]}"
    return None


def replay(oracle, fixture):
    """list of 'case k slot: what differs' over the whole fixture"""
    cases, _ = fixture
    bad = []
    for k, (case, rec) in enumerate(cases):
        got, intention, view = checker_calls(oracle, case)            # (no exception escapes: a raising checker fails the test)
        if not np.array_equal(SC.class_counts(view.cls), rec["counts"]):
            bad.append(f"case {k}: class counts {SC.class_counts(view.cls)} != {rec['counts']}")
        if rec["intention"] is not None and intention != rec["intention"]:
            bad.append(f"case {k}: intention {intention} != {rec['intention']}")
        for slot in SC.SLOTS:
            if rec["calls"][slot][0] == SC.NOT_RUN:
                continue
            if rec["calls"][slot][0] == SC.RAISES:
                why = continued(slot, got[slot], case, view)
                if why:
                    bad.append(f"case {k} {slot}: the reference raises {rec['calls'][slot][1]}, {why}")
                continue
            why = compare(rec["calls"][slot], got[slot], view)
            if why:
                bad.append(f"case {k} {slot}: {why}")
    return bad


def test_checker_returns_the_reference_decisions_on_every_recorded_scene(oracle, fixture):
    bad = replay(oracle, fixture)
    assert not bad, f"{len(bad)} differences, cases {sorted({int(b.split()[1].rstrip(':')) for b in bad})}:\n" + "\n".join(bad[:40])
