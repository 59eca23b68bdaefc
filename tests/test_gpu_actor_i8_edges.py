"""The controller's block fixed point on the device at the edges of its arithmetic, HIP == oracle bit for bit (-0 != +0, NaN == NaN): the
three kernels that contain npact8::actor8_body — np_actor_forward with the i8 buffer, np_policy_act with numerics 'i8' (actor and critic, the
critic with an edge recurrent state of its own), one PlanningEnv macro-step in the persistent schedule — and the fp32 kernels on the same rows.
Rows: tests/actor_i8_spec.py (edge rows of the recurrent state, found observation rows, non-finite rows, interleaved with ordinary rows so
that edge rows land in lanes 0 and 31 and in a ragged last tile); nets: the shipped one and the three synthetic ones; three chained calls, so
that edge outputs feed back.  What the oracle itself is worth: tests/test_actor_i8_spec_cpu.py.  Hit table: actor_i8_edges.json."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import actor_i8_spec as S  # noqa: E402
from oracle.f16_oracle import ActorOracle, PolicyOracle  # noqa: E402

NETS = ['shipped', 'weight_edges', 'flat_norms', 'steep_norms']
HITS = {}
REPORT = {}


def _sd(golden_dir, net):
    if net == 'shipped':
        d = np.load(f'{golden_dir}/actor_kat.npz')
        return {k[4:]: d[k] for k in d.files if k.startswith('sd::')}
    return S.synthetic_nets()[net]


def _rows(golden_dir):
    """(edge observations under the shipped LayerNorm 0, edge h, masks, non-finite rows) — built once."""
    from neuralplane_amd.actor import pack_ppo_actor
    if 'rows' not in HITS:
        w = pack_ppo_actor(_sd(golden_dir, 'shipped'))
        eo = S.edge_obs_rows(w)
        eh, em = S.edge_h_rows()
        ob, hh, _ = S.ordinary_rows(1, 99)
        HITS['rows'] = (eo, eh, em, S.nonfinite_rows(ob[0], hh[0]), S.classify_obs(w, eo), S.h_classes_of(eh, em))
    return HITS['rows']


def _classes_of(kinds, golden_dir):
    """The classes the rows of one batch reach: class -> rows."""
    eo, eh, em, nf, co, ch = _rows(golden_dir)
    t = {}
    for k in kinds:
        if k is None:
            continue
        names = {'h': lambda j: ch[j], 'obs': lambda j: co[j], 'extra': lambda j: {'nonfinite:' + nf[j][0]}}[k[0]](k[1])
        for c in names:
            t[c] = t.get(c, 0) + 1
    return t


def _add(table, more):
    for c, v in more.items():
        table[c] = table.get(c, 0) + v


def _assert_complete(kernel, table, wanted):
    """Every wanted class received rows in `kernel`; the table (counted inside ONE test, so it does not depend on which tests ran) joins the report."""
    from test_gpu_edge_cases import _write_report
    missing = [c for c in wanted if table.get(c, 0) < 1]
    assert not missing, (kernel, missing)
    REPORT[kernel] = table
    _write_report('actor_i8_edges.json', {'rows_per_class_and_kernel': REPORT, 'device_differs_from_oracle': 0})


def _all_classes(golden_dir):
    return S.H_CLASSES + S.OBS_CLASSES + ['nonfinite:' + r[0] for r in _rows(golden_dir)[3]]


def _flagged(obs, h, mask):
    """Rows the i8 contract turns into NaN: a non-finite observation, or a masked recurrent state holding an infinity, a NaN or 2^105 and more."""
    with np.errstate(all='ignore'):
        hm = np.abs(h * mask.reshape(-1, 1))
        return ~np.isfinite(obs).all(1) | ~(hm < 2.0 ** 105).all(1)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize('numerics', ['i8', 'fp32'])
@pytest.mark.parametrize('net', NETS)
def test_actor_forward_on_edge_and_non_finite_rows_equals_the_oracle(golden_dir, net, numerics, monkeypatch):
    """np_actor_forward at n = 33 and 97, three chained calls per batch (h_out feeds back, the edge observations stay).  i8: every flagged row is
    all NaN (the contract of f16_actor_i8.inc::ai8_row), whatever the sign and payload of its NaN.  fp32: both tilings; there ReLU maps NaN to 0,
    so non-finite observations give finite actions (an existing deviation from the reference) — pinned, not changed."""
    from neuralplane_amd.actor import FusedActor, pack_ppo_actor
    w = pack_ppo_actor(_sd(golden_dir, net))
    eo, eh, em, nf = _rows(golden_dir)[:4]
    o = ActorOracle(w, numerics)
    for n in (33, 97):
        table = {}
        for tile in ((0,) if numerics == 'i8' else (32, 64)):
            if tile:
                monkeypatch.setenv('NP_ACTOR_TILE', str(tile))
            fa = FusedActor(w, 'cuda:0', numerics=numerics)
            for obs, h, mask, kinds in S.batches(n, eo, eh, em, nf, seed=7):
                _add(table, _classes_of(kinds, golden_dir))
                h_o, h_t = h.copy(), _t(h.reshape(n, 1, 128))
                for call in range(3):
                    bad = _flagged(obs, h_o, mask)
                    a_t, _, h_t = fa(_t(obs), h_t, _t(mask.reshape(n, 1)))
                    a_o, h_o = o.forward(obs, h_o, mask)
                    assert S.same_bits(h_t.cpu().numpy()[:, 0], h_o), (n, tile, call, 'h_out')
                    assert S.same_bits(a_t.cpu().numpy(), a_o), (n, tile, call, 'actions')
                    if numerics == 'i8':
                        assert np.isnan(a_o[bad]).all() and np.isnan(h_o[bad]).all() and bad.sum() >= sum(k is not None and k[0] == 'extra' for k in kinds)
                        assert np.isfinite(a_o[~bad]).all() and np.isfinite(h_o[~bad]).all()
        if net == 'shipped':      # the found observation classes are defined under the shipped LayerNorm 0
            _assert_complete(f'np_actor_forward/{numerics}/n={n}', table, _all_classes(golden_dir))


@pytest.mark.parametrize('numerics', ['i8', 'fp32'])
@pytest.mark.parametrize('net', NETS)
def test_policy_act_on_edge_and_non_finite_rows_equals_the_oracle(golden_dir, net, numerics):
    """np_policy_act (FusedPolicy.get_actions): the actor takes the edge rows as they are, the critic the edge recurrent states in reverse
    order (an edge hc of its own); values, actions, log-probabilities and both recurrent states, three chained calls, n = 33 and 97."""
    from neuralplane_amd.policy import FusedPolicy, pack_policy_actor, pack_policy_critic
    from tests.policy_kat import random_state_dicts
    sa, sc = random_state_dicts(4, 5)
    sd = _sd(golden_dir, net)
    for k, v in sd.items():                       # the trunk of both networks from the net under test; heads and log_std stay random
        sa[k] = np.asarray(v, np.float32)
        kc = k.replace('act.mlp', 'mlp')
        if kc in sc:
            sc[kc] = np.asarray(v, np.float32)
    fp = FusedPolicy((sa, sc), 'cuda:0', numerics=numerics)
    o = PolicyOracle(pack_policy_actor(sa)[0], pack_policy_critic(sc), np.float32(fp.std), np.float32(fp.log_std), numerics)
    eo, eh, em, nf = _rows(golden_dir)[:4]
    for n in (33, 97):
        table = {}
        for obs, h, mask, kinds in S.batches(n, eo, eh, em, nf, seed=11):
            _add(table, _classes_of(kinds, golden_dir))
            ha_o, hc_o = h.copy(), h[::-1].copy()
            ha, hc = _t(ha_o.reshape(n, 1, 128)), _t(hc_o.reshape(n, 1, 128))
            eps = np.random.RandomState(n).normal(0, 1, (n, 4)).astype(np.float32)
            for call in range(3):
                bad_a, bad_c = _flagged(obs, ha_o, mask), _flagged(obs, hc_o, mask)
                v, a, lp, ha, hc = fp.get_actions(_t(obs), ha, hc, _t(mask.reshape(n, 1)), noise=_t(eps))
                ref = o.run(obs, ha_o, hc_o, mask, eps)
                for name, x, y in zip(('values', 'actions', 'logp', 'ha', 'hc'), (v, a, lp, ha, hc), ref):
                    assert S.same_bits(x.cpu().numpy().reshape(y.shape), y), (n, call, name)
                if numerics == 'i8':      # the contract, stated for the policy's two networks: actor rows and critic rows flagged on their own states
                    assert np.isnan(ref[1][bad_a]).all() and np.isnan(ref[2][bad_a]).all() and np.isnan(ref[3][bad_a]).all(), (n, call)
                    assert np.isnan(ref[0][bad_c]).all() and np.isnan(ref[4][bad_c]).all(), (n, call)
                    assert np.isfinite(ref[1][~bad_a]).all() and np.isfinite(ref[3][~bad_a]).all() and np.isfinite(ref[0][~bad_c]).all() and np.isfinite(ref[4][~bad_c]).all()
                ha_o, hc_o = ref[3], ref[4]
        if net == 'shipped':
            _assert_complete(f'np_policy_act/{numerics}/n={n}', table, _all_classes(golden_dir))


@pytest.mark.parametrize('net', NETS)
def test_planning_persistent_step_from_edge_recurrent_states_equals_the_oracle(golden_dir, net):
    """PlanningEnv macro-steps (50 controller calls each) in the persistent schedule at n = 33 with the i8 controller, its recurrent state
    (env.ego_rnn_states: the existing surface can set it) started from EVERY edge row whose mask is 1 — PlanningEnv always passes mask 1, so
    the class `masked_out` cannot occur here — and every non-finite recurrent state, in as many environments of 33 as that takes (edge rows in
    every second row and in lanes 0, 31 and 32).  Non-finite rows poison their aircraft by the spec's rule; the other rows of the tile are
    untouched.  Everything each step leaves behind, bit for bit; the hit table of this kernel is asserted complete."""
    from neuralplane_amd.actor import FusedActor, pack_ppo_actor
    from neuralplane_amd.envs.planning_env import PlanningEnv
    from tests.planning_closed import OracleClosedLoop
    from test_gpu_actor import _closed_result
    g0 = np.load(f'{golden_dir}/planning_closed_kat.npz')
    n = 33
    g = {'hi_actions': g0['hi_actions'][:, :n], 'rand_u_0': g0['rand_u_0'][:n]}
    w = pack_ppo_actor(_sd(golden_dir, net))
    eh, em, nf = _rows(golden_dir)[1:4]
    keep = [j for j in range(eh.shape[0]) if em[j] == 1]
    nf_h = [r for r in nf if r[0].startswith('h') and r[3] == 1.0]
    table, flagged_rows = {}, 0
    for obs_unused, h0, mask, kinds in S.batches(n, np.zeros((0, 22), np.float32), eh[keep], em[keep], nf_h, seed=3):
        assert (mask == 1).all()
        for k in kinds:
            if k is not None:
                names = _rows(golden_dir)[5][keep[k[1]]] if k[0] == 'h' else {'nonfinite:' + nf_h[k[1]][0]}
                _add(table, {c: 1 for c in names})
        bad = _flagged(np.zeros((n, 22), np.float32), h0, mask)
        flagged_rows += int(bad.sum())
        env = PlanningEnv(num_envs=n, config='tracking', model='F16', random_seed=0, device='cuda:0', controller=FusedActor(w, 'cuda:0', numerics='i8'))
        env.loop_mode, env.loop_waves, env.loop_block = 'persistent', 8, 0
        cl = OracleClosedLoop(g, w, 'i8')
        env._batch.reset(rand_u=g['rand_u_0'], want_obs=False)
        env.ego_rnn_states.copy_(_t(h0.reshape(env.ego_rnn_states.shape)))
        cl.h = h0.copy()
        got = _closed_result(env, env.step(_t(g['hi_actions'][0])))
        want = cl.macro_step(0)
        for q in ('flags', 'step_count', 's', 'u', 'tgt', 'rnn', 'obs', 'reward'):
            assert S.same_bits(np.asarray(got[q], np.float32), np.asarray(want[q], np.float32)), q
        assert np.isnan(want['rnn'][bad]).all() and np.isfinite(want['rnn'][~bad]).all()
    assert flagged_rows >= len(nf_h)
    _assert_complete(f'planning_persistent/i8/{net}', table, [c for c in S.H_CLASSES if c != 'masked_out'] + ['nonfinite:' + r[0] for r in nf_h])
