"""What the tests of the brake clearance by road users share (DESIGN.md §5.10 "Brake clearance by road users"): the seeded scenes of
tests/hidden_brake_scenes.py with a set of hidden road users ``(speed, metric, flow)``, the threshold table, ``map_of`` and -- by the
checkers alone -- one key map and one clearance per distinct ``(metric, flow)``.  Every scene carries a lane table, so all three
forecasts can be asked of the same class bytes."""
import copy

import numpy as np

import hidden_brake_classes_scenes as CS
import hidden_brake_scenes as SC
import ref_hidden_clearance as HC

FORECASTS = {("euclid", "any"): SC.ENTRIES[0], ("road", "any"): SC.ENTRIES[1], ("road", "lanes"): SC.ENTRIES[2]}
# a pedestrian anywhere on the road and as the crow flies, a cyclist along the road and along the lanes, a car along the lanes: 4 m/s on
# all three forecasts, so that the forecasts themselves can be told apart at one speed
USERS = ((1.5, "road", "any"), (4.0, "road", "lanes"), (4.0, "road", "any"), (4.0, "euclid", "any"), (8.0, "road", "lanes"))


def maps_of(users):
    """(the distinct (metric, flow) in order of first appearance, map_of [C])"""
    maps = []
    for _, metric, flow in users:
        if (metric, flow) not in maps:
            maps.append((metric, flow))
    return maps, [maps.index((metric, flow)) for _, metric, flow in users]


def user_scene(spec, users=USERS, maps=True):
    """the scene of ``spec`` (seed, M, T, entry, ragged -- the entry is not used: the users name their forecasts) with ``users`` (speeds
    scaled by hidden_brake_classes_scenes.speeds_for), ``tables``, ``thr [C, T]``, ``maps``, ``map_of``, ``r2_caps [K]`` = the end of the
    fastest table on each map and, with ``maps``, ``keys [K]`` and ``qmins [K]`` by the checkers"""
    sc = SC.scene(*spec)
    speeds = CS.speeds_for(sc.T, tuple(u[0] for u in users))
    sc.users = tuple((s, u[1], u[2]) for s, u in zip(speeds, users))
    sc.tables = CS.reach_tables(speeds, sc.T)
    sc.thr = CS.thresholds(sc.tables)
    sc.maps, sc.map_of = maps_of(sc.users)
    sc.r2_caps = [max(int(t[-1]) for t, k in zip(sc.tables, sc.map_of) if k == n) for n in range(len(sc.maps))]
    if maps:
        sc.keys, sc.qmins = [], []
        for forecast, r2_cap in zip(sc.maps, sc.r2_caps):
            key, qmin = forecast_maps(sc, forecast, r2_cap)
            sc.keys.append(key)
            sc.qmins.append(qmin)
    return sc


def forecast_maps(sc, forecast, r2_cap):
    """(key, qmin) of the scene under ``forecast`` = (metric, flow), by the clearance's checkers"""
    view = copy.copy(sc)
    view.entry = FORECASTS[forecast]
    key = CS.key_map(view, r2_cap)
    qmin = HC.clearance(key, sc.win, sc.road, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, SC.HL, SC.HW, SC.WB, sc.lens)
    return np.asarray(key), np.asarray(qmin)
