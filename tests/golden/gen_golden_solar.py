#!/usr/bin/env python3
"""Golden vectors for `solar`, recorded from the REFERENCE (build container only; stand-in for the un-vendored
earthkit-utils in tests/golden/_standin).  Writes tests/golden/solar_golden.npz, data only:
  * `index`: JSON -- the cases (function, dates as ISO strings, keyword arguments, the names of the input and output
    arrays, the Python type of the result), the node sets and the known answers of the reference's own tests;
  * per case the reference's output; for every f32 case also its output on the inputs upcast to f64 (`.up`);
  * per node set (interval, intervals_per_hour, integration_order): the dates the reference handed to its integrand and
    the weight of each (read off with a one-hot integrand), and julian_day, declination, time correction, incoming
    radiation and hour of every such date."""
import datetime as dt
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("EKM_REFERENCE", "/root/reference")
sys.path[:0] = [os.path.join(HERE, "_standin"), os.path.join(REF, "src")]

from earthkit.meteo.solar.array import solar as ref  # noqa: E402

np.seterr(all="ignore")
TZ1 = dt.timezone(dt.timedelta(hours=1))
TZM5 = dt.timezone(dt.timedelta(hours=-5, minutes=-30))

INSTANTS = {
    "known": dt.datetime(2024, 4, 22, 12, 0, 0),
    "minutes": dt.datetime(2023, 7, 15, 9, 37, 21),
    "tz": dt.datetime(2024, 4, 22, 12, tzinfo=TZ1),
    "tz_minutes": dt.datetime(2022, 10, 3, 17, 45, tzinfo=TZM5),
    "feb29": dt.datetime(2024, 2, 29, 6, 15),
    "dec31": dt.datetime(2023, 12, 31, 23, 59, 59),
    "jan1": dt.datetime(2024, 1, 1, 0, 0),
}
INTERVALS = {
    "known24h": (dt.datetime(2024, 4, 22), dt.timedelta(hours=24)),
    "minutes90min": (dt.datetime(2023, 7, 15, 9, 37), dt.timedelta(minutes=90)),
    "midnight3h": (dt.datetime(2024, 2, 29, 22, 30), dt.timedelta(hours=3)),
    "newyear3h": (dt.datetime(2023, 12, 31, 22, 10), dt.timedelta(hours=3)),
    "tz1h": (dt.datetime(2022, 10, 3, 17, 45, tzinfo=TZM5), dt.timedelta(hours=1)),
    "feb29_24h": (dt.datetime(2024, 2, 28, 18, 20), dt.timedelta(hours=24)),
}
# (intervals_per_hour, integration_order): 1 to 384 nodes over the intervals above
RULES = [(1, 3), (1, 1), (2, 2), (4, 4), (1, 4), (2, 3), (4, 1), (1, 2)]


def iso(d):
    return d.isoformat()


def points(rng, n):
    lat = rng.uniform(-90.0, 90.0, n)
    lon = rng.uniform(-360.0, 720.0, n)
    if n >= 4:
        lat[:2] = [90.0, -90.0]
        lon[2:4] = [-360.0, 720.0]
    return lat, lon


def main():
    store, cases, nodesets = {}, [], {}
    rng = np.random.default_rng(20261018)

    sets = {}
    for n in (1, 63, 64, 65, 257):
        sets[f"pts{n}"] = points(rng, n)
    special_lat = np.array([0.0, -0.0, 90.0, -90.0, 45.0, np.nan, 10.0, np.inf, -np.inf, 20.0, 20.0, np.nan, 90.0, -90.0, 89.999999, 30.0])
    special_lon = np.array([0.0, 180.0, 33.0, -33.0, np.nan, 12.0, np.inf, 7.0, 7.0, -np.inf, 540.0, np.nan, np.inf, np.nan, 719.5, -359.5])
    sets["special"] = (special_lat, special_lon)
    for name, (lat, lon) in sets.items():
        for tag, T in (("f64", np.float64), ("f32", np.float32)):
            store[f"in.{name}.{tag}.lat"], store[f"in.{name}.{tag}.lon"] = lat.astype(T), lon.astype(T)
    glat, glon = np.linspace(-90.0, 90.0, 5)[:, None], np.linspace(-180.0, 177.0, 67)[None, :]
    for tag, T in (("f64", np.float64), ("f32", np.float32)):
        store[f"in.grid.{tag}.lat"], store[f"in.grid.{tag}.lon"] = glat.astype(T), glon.astype(T)
    store["in.int.lat"], store["in.int.lon"] = np.array([-60, 0, 45, 90]), np.array([-170, 0, 18, 400])

    def record(func, when, pts, tag, kwargs=None, lat=None, lon=None, note=""):
        kwargs = kwargs or {}
        cid = f"{func}.{when}.{pts}.{tag}" + "".join(f".{k[:3]}{v}" for k, v in sorted(kwargs.items()))
        if lat is None:
            lat, lon = store[f"in.{pts}.{tag}.lat"], store[f"in.{pts}.{tag}.lon"]
            lat_key, lon_key = f"in.{pts}.{tag}.lat", f"in.{pts}.{tag}.lon"
        else:
            lat_key = lon_key = None
        if func == "instant":
            dates = [INSTANTS[when]]
            call = lambda a, b: ref.cos_solar_zenith_angle(dates[0], a, b)  # noqa: E731
        else:
            begin, span = INTERVALS[when]
            dates = [begin, begin + span]
            fn = ref.cos_solar_zenith_angle_integrated if func == "integrated" else ref.toa_incident_solar_radiation
            call = lambda a, b: fn(dates[0], dates[1], a, b, **kwargs)  # noqa: E731
        out = call(lat, lon)
        case = dict(id=cid, func=func, dates=[iso(d) for d in dates], kwargs=kwargs, lat=lat_key, lon=lon_key, note=note,
                    result_type=type(out).__name__, dtype=str(np.asarray(out).dtype), shape=list(np.shape(out)))
        if lat_key is None:
            case["lat_value"], case["lon_value"] = lat, lon
        store[f"out.{cid}"] = np.asarray(out)
        if tag == "f32":
            store[f"out.{cid}.up"] = np.asarray(call(np.asarray(lat).astype(np.float64), np.asarray(lon).astype(np.float64)))
        cases.append(case)

    for tag in ("f64", "f32"):
        for when in INSTANTS:
            for pts in ("pts65", "special"):
                record("instant", when, pts, tag)
        for pts in ("pts1", "pts63", "pts64", "pts257", "grid"):
            record("instant", "minutes", pts, tag)
        for func in ("integrated", "toa"):
            for when in INTERVALS:
                for iph, order in RULES:
                    record(func, when, "pts65", tag, dict(intervals_per_hour=iph, integration_order=order))
                record(func, when, "special", tag)
            for pts in ("pts1", "pts63", "pts64", "pts257"):
                record(func, "known24h", pts, tag)
    # integer input (instantaneous only: the integrated functions raise), Python scalars: the reference's known answers
    out = ref.cos_solar_zenith_angle(INSTANTS["known"], store["in.int.lat"], store["in.int.lon"])
    store["out.instant.known.int"] = np.asarray(out)
    cases.append(dict(id="instant.known.int", func="instant", dates=[iso(INSTANTS["known"])], kwargs={}, lat="in.int.lat",
                      lon="in.int.lon", note="integer input", result_type=type(out).__name__, dtype=str(out.dtype),
                      shape=list(out.shape)))
    record("instant", "known", "scalar", "py", lat=40.0, lon=18.0, note="known answer 0.8478445449796352")
    for order in (1, 2, 3, 4):
        record("integrated", "known24h", "scalar", "py", dict(integration_order=order), lat=40.0, lon=18.0, note="known answer 0.3110738757")
    record("toa", "known24h", "scalar", "py", lat=40.0, lon=18.0, note="known answer 1503617.8237746414")

    # node sets: what the reference's _integrate hands to its integrand
    for when, (begin, span) in INTERVALS.items():
        for iph, order in RULES:
            seen = []

            def count(date, la, lo):
                seen.append(date)
                return np.zeros_like(la)

            kw = dict(intervals_per_hour=iph, integration_order=order)
            ref._integrate(count, begin, begin + span, np.zeros(1), np.zeros(1), **kw)
            n, k = len(seen), [0]

            def one_hot(date, la, lo):
                e = np.zeros(n)
                e[k[0]] = 1.0
                k[0] += 1
                return e

            w = ref._integrate(one_hot, begin, begin + span, np.zeros(n), np.zeros(n), **kw)
            key = f"{when}.iph{iph}.ord{order}"
            nodesets[key] = dict(begin=iso(begin), end=iso(begin + span), kwargs=kw, dates=[iso(d) for d in seen])
            store[f"nodes.{key}.w"] = np.asarray(w)
            store[f"nodes.{key}.jd"] = np.array([ref.julian_day(d) for d in seen])
            store[f"nodes.{key}.decl"] = np.array([ref.solar_declination_angle(d)[0] for d in seen])
            store[f"nodes.{key}.tc"] = np.array([ref.solar_declination_angle(d)[1] for d in seen])
            store[f"nodes.{key}.isr"] = np.array([ref.incoming_solar_radiation(d) for d in seen])
            store[f"nodes.{key}.hour"] = np.array([d.hour for d in seen])
    scalars = {}
    for name, d in INSTANTS.items():
        dec, tc = ref.solar_declination_angle(d)
        scalars[name] = dict(date=iso(d), julian_day=float(ref.julian_day(d)).hex(), declination=float(dec).hex(),
                             time_correction=float(tc).hex(), isr=float(ref.incoming_solar_radiation(d)).hex())
    known = dict(julian_day=[[iso(dt.datetime(2024, 4, 22)), 112.0], [iso(INSTANTS["known"]), 112.5], [iso(INSTANTS["tz"]), 112.5]],
                 declination=[[iso(dt.datetime(2024, 4, 22)), [12.235799080498582, 0.40707190497656276]],
                              [iso(INSTANTS["known"]), [12.403019177270453, 0.43253901867797273]]],
                 isr=[[iso(INSTANTS["known"]), 4833557.3088814365]],
                 cos_sza=0.8478445449796352, integrated=0.3110738757, toa=1503617.8237746414)
    index = dict(cases=cases, nodesets=nodesets, scalars=scalars, known=known, numpy=np.__version__)
    store["index"] = np.frombuffer(json.dumps(index).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "solar_golden.npz")
    np.savez_compressed(path, **store)
    print("wrote", len(store), "arrays,", len(cases), "cases,", len(nodesets), "node sets,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
