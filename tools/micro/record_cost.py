"""What recording costs inside mhip_vv_run (fp32), through the C ABI: ms/step of the 256k-atom LJ fluid and of 6mrr with PME at 0.5 fs, in one process, REPEATS
alternating windows of N steps each, of
  (a)  the plain run;
  (b)  the recorded run with the kinetic energy every 10 steps;
  (c)  (b) plus coordinates every 100 steps;
  (d)  the host-chunked loop making the same reads through the entry points that exist without the recorder: mhip_vv_run per chunk, then mhip_kinetic_energy
       (d_b: the reads of b) and mhip_get_state of the coordinates every 100 steps (d_c: the reads of c).
Every form has a context of its own, warmed up; the recorded forms read their history back inside the timed window.  Printed per form: the median and the spread;
per system: (b) − (a) per record beside the 5 µs dispatch floor, and whether the medians of (b), (c) are at or below (d)'s.
Then a frame on its own: µs per coordinate record of mhip_record_now, FRAMES records behind one synchronisation (the figure the scatter-write through orig inside
k_record was chosen by, against a gather-read through inv in a launch of its own: DESIGN §10i).
(for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/micro/record_cost.py 500 1)"""
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import molly_loader  # noqa: E402

m = molly_loader.load()
W = importlib.import_module("molly_jl_amd.workloads")
L = m.lib()
T = np.float32
N = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
FRAMES = 50
KE_EVERY, X_EVERY, WARM = 10, 100, 500
SYSTEMS = {
    "lj256k": (lambda: W.lj_fluid(64, seed=2, dtype=T), 0.002),
    "6mrr_pme_0.5fs": (lambda: W.protein_6mrr("ewald", T, pme=True), 0.0005),
}
p = lambda a: a.ctypes.data_as(C.c_void_p)


def context(case):
    s = case.system(m, T)
    s.push_state(velocities=True)
    return s


def set_record(s, every, capacity):
    s._check(L.mhip_set_record(s._ctx, C.byref((C.c_int32 * 4)(*every)), C.byref((C.c_int64 * 4)(*capacity))))


def window(s, form, first, dt, bufs):
    """one timed window of N steps from `first` → ms/step"""
    ke, frame, d = bufs["ke"], bufs["frame"], C.c_double(0)
    t = time.perf_counter()
    if form == "a":
        s._check(L.mhip_vv_run(s._ctx, first, N, dt, 1))
    elif form in ("b", "c"):
        s._check(L.mhip_record_clear(s._ctx))
        s._check(L.mhip_vv_run(s._ctx, first, N, dt, 1))
        s._check(L.mhip_record_read(s._ctx, 0, 0, N // KE_EVERY, None, p(ke), 0))
        if form == "c":
            for k in range(N // X_EVERY):      # (one frame buffer on the host, as the chunked loop has)
                s._check(L.mhip_record_read(s._ctx, 2, k, 1, None, p(frame), 0))
    else:
        for k in range(N // KE_EVERY):
            s._check(L.mhip_vv_run(s._ctx, first + k * KE_EVERY, KE_EVERY, dt, 1))
            s._check(L.mhip_kinetic_energy(s._ctx, C.byref(d)))
            ke[k] = d.value
            if form == "d_c" and (first + (k + 1) * KE_EVERY) % X_EVERY == 0:
                s._check(L.mhip_get_state(s._ctx, p(frame), None, 0))
    return 1e3 * (time.perf_counter() - t) / N


for name, (make, dt) in SYSTEMS.items():
    case = make()
    bufs = dict(ke=np.zeros(N // KE_EVERY), frame=np.zeros((case.n, 3), T))
    runs = {}
    for form in ("a", "b", "c", "d_b", "d_c"):
        s = context(case)
        if form == "b":
            set_record(s, [KE_EVERY, 0, 0, 0], [N // KE_EVERY, 0, 0, 0])
        if form == "c":
            set_record(s, [KE_EVERY, 0, X_EVERY, 0], [N // KE_EVERY, 0, N // X_EVERY, 0])
        s._check(L.mhip_vv_run(s._ctx, 0, WARM, dt, 1))
        runs[form] = (s, [])
    for r in range(REPEATS):
        for form, (s, ms) in runs.items():
            ms.append(window(s, form, WARM + r * N, dt, bufs))
    med = {form: statistics.median(ms) for form, (s, ms) in runs.items()}
    for form, (s, ms) in runs.items():
        print(dict(system=name, form=form, ms_per_step_median=round(med[form], 5), spread=[round(x, 5) for x in ms], fused_steps=s.stats()["n_fused_steps"]), flush=True)
    print(dict(system=name, us_per_ke_record=round(1e3 * (med["b"] - med["a"]) * KE_EVERY, 2), dispatch_floor_us=5.0,
               us_per_frame_record=round(1e3 * (med["c"] - med["b"]) * X_EVERY, 2), b_not_above_d=med["b"] <= med["d_b"], c_not_above_d=med["c"] <= med["d_c"],
               chunked_over_recorded=(round(med["d_b"] / med["b"], 3), round(med["d_c"] / med["c"], 3))), flush=True)
    del runs

    # one frame on its own: FRAMES coordinate records of mhip_record_now, timed behind one synchronisation
    s = context(case)
    s._check(L.mhip_vv_run(s._ctx, 0, 20, dt, 1))   # a sorted order that is not the caller's
    set_record(s, [0, 0, 1, 0], [0, 0, FRAMES, 0])
    us = []
    for r in range(REPEATS + 1):
        s._check(L.mhip_record_clear(s._ctx))
        s._check(L.mhip_synchronize(s._ctx))
        t = time.perf_counter()
        for k in range(FRAMES):
            s._check(L.mhip_record_now(s._ctx, 20, 1 << 2))
        s._check(L.mhip_synchronize(s._ctx))
        if r:      # (the first round warms up)
            us.append(1e6 * (time.perf_counter() - t) / FRAMES)
    print(dict(system=name, us_per_frame=round(statistics.median(us), 2), spread=[round(x, 2) for x in us]), flush=True)
    del s
