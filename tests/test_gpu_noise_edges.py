"""The observation-noise generator on the device at the edges of its index range and of its counter packing, HIP == oracle bit
for bit (what the oracle's generator is worth is tests/test_noise_spec_cpu.py: every index against fp64).

* Edge draws.  A given pair draws one of the 8 lowest radius indices once per 2^18 rows, so the ordinary tests have very likely
  never evaluated the device twins there — np_f16_device.h::noise_pair (scalar, per Philox block, through LDS in the latency family)
  and np_math.h::*_spec2 (packed two-wide; pair 10 scalar).  The host scans a few million rows of one (seed, call) for rows in which
  a pair of each group ({0..7} top bits packed, {8, 9} low bits packed, {10} low bits scalar) falls in each class: K1 < 8 (5.5 sigma),
  K1 >= 2^21 - 8 (w = 4.8e-7, the lower end of sqrt_spec's domain), K1 within 4 of a seam of neg2ln_spec (u = sqrt(1/2) 2^e) or of
  the index of the largest fp64 error, base angle < 8 or >= 2^18 - 8.  Every cell must be hit; the batch is then placed so that the
  row sits mid-wave (row0 = R - 17) and the reset kernel's observation and one step are compared with the oracle, noise_scale 1.
* Counter packing.  rng_block packs call_idx >> 32 into 24 bits under the block number, adds a device-side base for launches
  replayed from a HIP graph, and splits the 64-bit global row over two words: call indices at and across 2^32, 2^40 and 2^56 (bits
  >= 56 are dropped by the spec: both sides must wrap alike), host index + device base crossing 2^32 inside a graph replay, and
  global rows crossing 2^32 inside one wave.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from noise_spec import CENTRES, GROUPS, edge_classes, find_edge_rows  # noqa: E402
from oracle import f16_oracle as fo  # noqa: E402
from oracle.f16_oracle import Oracle  # noqa: E402  (the checker; test infrastructure)
from test_gpu_edge_cases import VARIANTS, _check, _load, _mk, _same, _write_report  # noqa: E402

N = 64
SEED, CALL = 77, 12345
SCAN_START, SCAN_ROWS = 1000, 4_000_000
NOISE_ON = {'noise_scale': 1.0}       # no noise bit disappears under the observation's rounding
_HITS = []


def _edge_hits():
    if not _HITS:
        _HITS.extend(find_edge_rows(SEED, CALL, SCAN_START, SCAN_ROWS))
    return _HITS


def test_every_edge_class_is_hit_in_every_pair_group():
    hits = _edge_hits()
    k1, k2 = fo.noise_indices_rows(SEED, CALL, 0, 1)
    classes = list(edge_classes(k1, k2))
    assert len(classes) == 6
    table = {c: {g: [h for h in hits if h['class'] == c and h['group'] == g] for g in GROUPS} for c in classes}
    # the hit table (class, group, row, pair, K per hit) as noise_edges.json next to the division self-check's report
    _write_report('noise_edges.json', {'seed': SEED, 'call_idx': CALL, 'rows_scanned': [SCAN_START, SCAN_START + SCAN_ROWS], 'hits': hits})
    for c in classes:
        for g in GROUPS:
            assert 1 <= len(table[c][g]) <= 3, f'no row with a pair of group {g} in class {c}'
            # the pooled classes (four seams, two arg-max indices) through as many different neighbourhoods as three rows can hold
            assert len({h['centre'] for h in table[c][g]}) == min(3, len(CENTRES[c]()) if c in CENTRES else 1), (c, g)
    for h in hits:          # the scan's verdict, re-derived for the single row
        a, b = fo.noise_indices_rows(SEED, CALL, h['row'], 1)
        mask, k = edge_classes(a, b)[h['class']]
        assert mask[0, h['pair']] and int(k[0, h['pair']]) == h['K'] and h['pair'] in GROUPS[h['group']] and h['row'] >= SCAN_START


def _loaded(task, variant, seed=SEED):
    """A batch of N and the oracle's state, both holding the same freshly initialised aircraft with all flags clear."""
    b, o = _mk(task, N, variant, overrides=NOISE_ON, seed=seed)
    st = Oracle.new_state(N)
    o.reset(st, seed=seed, call_idx=0, want_obs=False)
    _load(b, st)
    return b, o, st


@pytest.mark.parametrize('task,variant', [('heading', v) for v in VARIANTS] + [('control', 'latency'), ('control', 'pair')])
def test_edge_draws_in_the_reset_and_the_step_kernel(task, variant):
    hits = _edge_hits()
    rows = sorted({h['row'] for h in hits})
    assert rows and rows[0] >= 17
    b, o, st0 = _loaded(task, variant)
    o_clean = Oracle(task, overrides={'noise_scale': 0.0})
    rng = np.random.RandomState(5)
    noisy = 0
    for R in rows:
        st = {k: v.copy() for k, v in st0.items()}
        _load(b, st)
        b.row0, b.call_idx = R - 17, CALL
        obs = b.observe().cpu().numpy()                     # the reset kernel on clear flags: the observation of the loaded state
        o_obs = o.reset(st, seed=SEED, call_idx=CALL, row0=R - 17)
        assert _same(obs, o_obs), f'{task} {variant}: observation, edge row {R}'
        # what was compared carries the edge row's 22 draws at full scale in row 17: observation - clean observation == z to the
        # one rounding of the fma and the one of this difference
        z = fo.rng_normals_rows(SEED, CALL, R, 1)[0].astype(np.float64)
        clean = o_clean.reset({k: v.copy() for k, v in st0.items()}, seed=SEED, call_idx=CALL, row0=R - 17)[17].astype(np.float64)
        assert np.all(np.abs((obs[17] - clean) - z) <= 2.0 ** -22 * (np.abs(clean) + np.abs(z))), f'{task} {variant}: row {R} does not carry its draws'
        noisy += int(np.abs(z).max() > 3.5)                # K1 < 8: r > 4.99, and the larger of |cos|, |sin| is at least 0.707
        # one step on the same rows and the same call: the same draws, placed by the step kernel
        a = rng.uniform(-1.0, 1.0, (N, 4)).astype(np.float32)
        b.call_idx = CALL
        obs, rew, flags = b.step(torch.from_numpy(a).cuda())
        o_obs, o_rew, _, _, _ = o.step(st, a, seed=SEED, call_idx=CALL, row0=R - 17)
        _check(b, obs, rew, flags, st, o_obs, o_rew, f'{task} {variant}: step, edge row {R}')
    assert noisy >= 3, 'the K1 < 8 rows must show a draw beyond 3.5 sigma'


COUNTER_VARIANTS = ['latency8', 'pair']


@pytest.mark.parametrize('variant', COUNTER_VARIANTS)
@pytest.mark.parametrize('call0', [2 ** 32 - 2, 2 ** 40 + 5, 2 ** 56 - 3])
def test_call_index_at_and_across_2_32_2_40_and_2_56(call0, variant):
    b, o, st = _loaded('heading', variant, seed=3)
    rng = np.random.RandomState(1)
    b.call_idx = call0
    for t in range(4):
        a = rng.uniform(-1.0, 1.0, (N, 4)).astype(np.float32)
        obs, rew, flags = b.step(torch.from_numpy(a).cuda())
        o_obs, o_rew, _, _, _ = o.step(st, a, seed=3, call_idx=call0 + t)
        _check(b, obs, rew, flags, st, o_obs, o_rew, f'{variant}: call_idx {call0} + {t}')
    assert b.call_idx == call0 + 4
    if call0 >= 2 ** 56 - 3:      # bits >= 56 are dropped: the stream of call 2^56 + 1 is the stream of call 1
        assert np.array_equal(fo.rng_normals_rows(3, 2 ** 56 + 1, 0, 4), fo.rng_normals_rows(3, 1, 0, 4))
    assert not np.array_equal(fo.rng_normals_rows(3, 2 ** 32 + 1, 0, 4), fo.rng_normals_rows(3, 1, 0, 4))


@pytest.mark.parametrize('variant', COUNTER_VARIANTS)
def test_global_rows_cross_2_32_inside_one_wave(variant):
    row0 = 2 ** 32 - 30
    b, o = _mk('heading', N, variant, overrides=NOISE_ON, seed=8)
    b.row0 = row0
    st = Oracle.new_state(N)
    rng = np.random.RandomState(2)
    obs = b.reset()                                          # every row initialised from the uniforms of its global row
    o_obs = o.reset(st, seed=8, call_idx=0, row0=row0)
    _check(b, obs, torch.zeros(N), b.flags, st, o_obs, np.zeros(N, np.float32), f'{variant}: reset')
    for t in range(3):
        a = rng.uniform(-1.0, 1.0, (N, 4)).astype(np.float32)
        obs, rew, flags = b.step(torch.from_numpy(a).cuda())
        o_obs, o_rew, _, _, _ = o.step(st, a, seed=8, call_idx=t + 1, row0=row0)
        _check(b, obs, rew, flags, st, o_obs, o_rew, f'{variant}: step {t}')
    z = fo.rng_normals_rows(8, 1, row0, N)
    assert not np.array_equal(z[30:], fo.rng_normals_rows(8, 1, 0, N - 30)), 'row 2^32 must not draw what row 0 draws'


@pytest.mark.parametrize('variant', COUNTER_VARIANTS)
def test_host_call_index_plus_device_base_crosses_2_32_in_a_graph_replay(variant):
    """np_f16_io.call_idx_base: two step launches captured in one HIP graph (F16Batch.launch_static, the route PlanningEnv's graph
    mode takes) with host offsets 0 and 1 and the base on the device; the base starts at 2^32 - 3 and advances by 2 per replay, so the
    second replay has base 2^32 - 1 + offset 1 = 2^32 (the carry happens in the kernel's add) and the third starts beyond."""
    b, o, st = _loaded('heading', variant, seed=6)
    d = b.device
    fa, fb = b.flags.clone(), torch.empty_like(b.flags)
    act = [torch.zeros((N, 4), device=d) for _ in range(2)]
    obs = [torch.empty((N, 22), device=d) for _ in range(2)]
    rew = [torch.empty(N, device=d) for _ in range(2)]

    def body():
        b.launch_static(fa, fb, 0, action=act[0], obs=obs[0], reward=rew[0], cache_valid=False)
        b.launch_static(fb, fa, 1, action=act[1], obs=obs[1], reward=rew[1], cache_valid=True)
        b.call_base.add_(2)

    side = torch.cuda.Stream(device=d)                      # warm-up outside the capture, then the state is loaded again
    side.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(side), torch.no_grad():
        body()
    torch.cuda.current_stream(d).wait_stream(side)
    torch.cuda.synchronize()
    _load(b, st)
    fa.copy_(b.flags)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        body()
    base = 2 ** 32 - 3
    b.call_base.fill_(base)
    rng = np.random.RandomState(4)
    for k in range(3):
        a = [rng.uniform(-1.0, 1.0, (N, 4)).astype(np.float32) for _ in range(2)]
        for j in range(2):
            act[j].copy_(torch.from_numpy(a[j]))
        graph.replay()
        torch.cuda.synchronize()
        for j in range(2):
            o_obs, o_rew, _, _, _ = o.step(st, a[j], seed=6, call_idx=base + 2 * k + j)
            assert _same(obs[j].cpu().numpy(), o_obs) and _same(rew[j].cpu().numpy(), o_rew), f'{variant}: replay {k} launch {j}'
        _check(b, obs[1], rew[1], fa, st, o_obs, o_rew, f'{variant}: replay {k}')
    assert int(b.call_base.item()) == base + 6 and base + 6 > 2 ** 32
