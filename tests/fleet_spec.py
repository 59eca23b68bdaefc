"""Shared by the CPU and GPU suites of the fleet (per-row airframes; test infrastructure): the airframe classes, the index patterns, the
actions, and the EXPECTED VALUE of a mixed batch — the CPU oracle as it stands, run once per class on all rows (same seed, row0, actions), rows
picked by class.  Rows are independent and the RNG is keyed by global row, so that construction is exact: row i of a fleet must equal row i of
Oracle(task, airframe=class of row i) bit for bit."""
import numpy as np

from oracle.f16_oracle import Oracle

N = 293            # two 128-row tiles + a ragged tail: a full tile, a tile boundary and a partial tile
STEPS = 40
SEED, ROW0 = 1234, 7_000_000_000
# three classes: the F-16; a heavier one with more pitch inertia; one that moves the c.g., the wing area, the thrust and the atmosphere lapse
CLASSES = [{}, {'mass': 700, 'Jy': 60000}, {'xcg': 0.25, 'S': 320.0, 'thrust_max': 60000.0, 'atm_lapse': 0.65e-5}]
TWO = CLASSES[:2]


def mixed_index(n=N, k=3):
    """rows 0..191: i % k, so the classes mix inside every wave; rows 192..255: one wave of class 1 alone; then a run of class k-1; the last
    rows mixed again.  (At N = 293 the fifth wave is the ragged tail, so the run of class k-1 and the mixed tail share it: rows 256..287 and
    288..292.)"""
    idx = np.arange(n, dtype=np.int32) % k
    idx[192:256] = 1
    idx[256:288] = k - 1
    return idx


def actions(t, rng, n=N):
    """the hazard-rich actions of tests/test_gpu_gemm_order.py: episodes end all along the run"""
    a = rng.uniform(-1.5, 1.5, (n, 4)).astype(np.float32)
    a[:, 1] *= 3.0 if t % 7 == 0 else 1.0
    return a


def snapshot(st, obs, rew):
    return ({k: np.array(v, copy=True) for k, v in st.items()}, None if obs is None else np.array(obs, copy=True), None if rew is None else np.array(rew, copy=True))


_RUNS = {}


def class_run(task, solver, airframe, steps=STEPS, n=N, row0=ROW0):
    """reset + `steps` free-running steps of ONE class on all n rows: [(state dict, obs, reward)] after every call.  Computed once per key."""
    key = (task, solver, tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in airframe.items())), steps, n, row0)
    if key not in _RUNS:
        o = Oracle(task, solver=solver, overrides={'airframe': dict(airframe)} if airframe else None)
        st = Oracle.new_state(n)
        rng = np.random.RandomState(5)
        out = [snapshot(st, o.reset(st, seed=SEED, call_idx=0, row0=row0), None)]
        for t in range(steps):
            o_obs, o_rew, _, _, _ = o.step(st, actions(t, rng, n), seed=SEED, call_idx=t + 1, row0=row0)
            out.append(snapshot(st, o_obs, o_rew))
        _RUNS[key] = out
    return _RUNS[key]


def select(snaps, index):
    """[(state, obs, reward) of class c on all rows] per class, index[n] -> the mixed batch's (state, obs, reward): row i from class index[i]"""
    st = {k: np.array(snaps[0][0][k], copy=True) for k in snaps[0][0]}
    obs = None if snaps[0][1] is None else np.array(snaps[0][1], copy=True)
    rew = None if snaps[0][2] is None else np.array(snaps[0][2], copy=True)
    for c in range(1, len(snaps)):
        rows = index == c
        for k in st:
            st[k][rows] = snaps[c][0][k][rows]
        if obs is not None:
            obs[rows] = snaps[c][1][rows]
        if rew is not None:
            rew[rows] = snaps[c][2][rows]
    return st, obs, rew


def expected_run(task, solver, classes, index, steps=STEPS, n=N, row0=ROW0):
    """the mixed batch after every call, and the number of auto-resets per class inside the window (flags raised by steps 1 .. steps-1)"""
    runs = [class_run(task, solver, c, steps, n, row0) for c in classes]
    out = [select([r[t] for r in runs], index) for t in range(steps + 1)]
    resets = []
    for c in range(len(classes)):
        rows = index == c
        resets.append(int(sum(((st['done'][rows] != 0) | (st['bad'][rows] != 0) | (st['timeout'][rows] != 0)).sum() for st, _, _ in out[1:steps])))
    return out, resets


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def state_bits_differ(a, b):
    """per row: do the two [n, 12] states differ in any bit?"""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) != np.ascontiguousarray(b, np.float32).view(np.uint32)).any(axis=1)
