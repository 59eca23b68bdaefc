"""CPU tests of the host-side mirror of the reference interface (no GPU, no kernels)."""
import numpy as np
import pytest
import torch
import yaml

from neuralplane_amd import sharding
from neuralplane_amd.core import cfg_from_config
from neuralplane_amd.envs.utils.utils import parse_config, wrap_PI


def test_parse_config_contract():
    c = parse_config('heading')
    assert c.dt == 0.02 and c.solver == 'euler' and c.num_observation == 22 and c.num_actions == 4
    assert c.init_state['init_T'] == 2000 and c.max_check_interval == 2500 and c.min_check_interval == 300
    assert getattr(c, 'does_not_exist', 7) == 7          # read with getattr(config, key, default)
    with pytest.raises(AssertionError):
        parse_config('no_such_scenario')                 # envs/utils/utils.py:22-23
    assert parse_config('tracking').noise_scale == 0 and parse_config('tracking').num_actions == 3
    assert parse_config('control').max_pitch_increment == 3


def test_cfg_defaults_follow_the_reference_getattr_calls():
    bag = type('EnvConfig', (object,), {'init_state': {'init_T': 1500}})
    c = cfg_from_config(bag, 'control')
    assert (c.dt, c.noise_scale, c.altitude_limit, c.acceleration_limit) == (0.02, 0.01, 2500.0, 300.0)
    assert (c.max_check_interval, c.min_check_interval) == (1500, 300)   # unreach_heading.py:16-17 defaults
    assert (c.max_altitude, c.min_altitude, c.max_vt, c.min_vt) == (20000, 19000, 1200, 1000)
    assert (c.max_heading_increment, c.max_pitch_increment, c.max_velocities_u_increment) == (0.3, 0.3, 100)
    assert c.init_T == 1500 and c.task == 1 and c.solver == 0
    with pytest.raises(NotImplementedError):
        cfg_from_config(type('C', (object,), {'init_state': {'init_T': 1}, 'solver': 'dopri5'}), 'heading')


def test_scenario_yaml_keys_are_complete():
    import os
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'neuralplane_amd', 'envs', 'configs')
    need = {'airspeed', 'noise_scale', 'solver', 'dt', 'num_agents', 'num_states', 'num_controls', 'num_actions',
            'num_observation', 'altitude_limit', 'acceleration_limit', 'max_velocity', 'min_velocity', 'min_alpha',
            'max_alpha', 'min_beta', 'max_beta', 'max_check_interval', 'min_check_interval', 'init_state',
            'max_altitude', 'min_altitude', 'max_vt', 'min_vt'}
    for name in ('heading', 'control', 'tracking'):
        y = yaml.safe_load(open(os.path.join(d, name + '.yaml')))
        assert need <= set(y), need - set(y)


def test_control_env_errors_match_the_reference():
    from neuralplane_amd.envs.control_env import ControlEnv
    with pytest.raises(NotImplementedError):
        ControlEnv(num_envs=2, config='heading', model='UAV', random_seed=0, device='cuda:0')   # control_env.py:26-27
    with pytest.raises(AssertionError):
        ControlEnv(num_envs=2, config='nope', model='F16', random_seed=0, device='cuda:0')


def test_gpuvecenv_reshapes_like_the_reference():
    """GPUVecEnv contract (env_wrappers.py:84-123) exercised on a stub env (CPU tensors)."""
    from neuralplane_amd.envs.env_wrappers import GPUVecEnv

    class Stub:
        num_envs, num_agents, n, device = 6, 1, 6, torch.device('cpu')
        observation_space = action_space = None

        def reset(self):
            return torch.arange(6 * 22, dtype=torch.float32).reshape(6, 22)

        def step(self, a):
            assert a.shape == (6, 4) and a.dtype == torch.float32
            z = torch.zeros(6, dtype=torch.bool)
            return self.reset() + a[:, :1], a.sum(1), z, ~z, z, {}

    v = GPUVecEnv([Stub])
    assert v.reset().shape == (6, 1, 22)
    obs, rew, done, bad, tmo, info = v.step(np.ones((6, 1, 4), np.float32))
    assert obs.shape == (6, 1, 22) and rew.shape == (6, 1, 1) and done.shape == bad.shape == tmo.shape == (6, 1, 1)
    assert rew.dtype == np.float32 and done.dtype == np.bool_ and bad.all() and not done.any() and info == {}
    with pytest.raises(AssertionError):
        GPUVecEnv([Stub, Stub])
    # VecEnv protocol of the reference (env_wrappers.py:40-82,113-123): step == step_async + step_wait, close() is idempotent
    assert v.closed is False
    v.step_async(np.ones((6, 1, 4), np.float32))
    obs2 = v.step_wait()[0]
    assert np.array_equal(obs2, obs)
    with pytest.raises(RuntimeError):
        v.step_wait()
    v.close()
    v.close()
    assert v.closed is True
    with pytest.raises(RuntimeError):
        v.step_async(np.ones((6, 1, 4), np.float32))


def test_shipped_yaml_constants_equal_the_reference():
    """neuralplane_amd/envs/configs/*.yaml are re-written files; their key/value sets must equal the reference's
    (envs/configs/*.yaml, algorithms/pid/config/*.yaml), recorded by tools/gen_yaml_fixture.py in the build container."""
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ref = json.load(open(os.path.join(root, 'tests', 'golden', 'ref_yaml_configs.json')))
    cfg = os.path.join(root, 'neuralplane_amd', 'envs', 'configs')
    assert set(ref['scenarios']) == {'heading', 'control', 'tracking', 'selfplay'}
    for name, want in ref['scenarios'].items():
        got = yaml.safe_load(open(os.path.join(cfg, name + '.yaml')))
        assert got == want, (name, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)})
        bag = parse_config(name)
        for k, v in want.items():
            assert getattr(bag, k) == v
    for name, want in ref['pid'].items():
        assert yaml.safe_load(open(os.path.join(cfg, 'pid', name + '.yaml'))) == want, name


def test_spaces_are_boxes_with_shape():
    from neuralplane_amd.envs.spaces import Box
    b = Box(low=-np.inf, high=np.inf, shape=(22,))
    assert b.shape == (22,)


def test_wrap_pi_helper():
    x = torch.tensor([0.0, 3.5, -3.5, 7.0, -7.0, 100.0])
    w = wrap_PI(x)
    assert torch.all(w <= torch.pi + 1e-6) and torch.all(w > -torch.pi - 1e-6)
    assert torch.allclose(torch.sin(w), torch.sin(x), atol=1e-5)


def test_shard_rows_partitions_exactly():
    for n_total, world in [(8_000_000, 8), (1000, 3), (7, 8), (256, 1)]:
        spans = [sharding.shard_rows(n_total, world, r) for r in range(world)]
        assert spans[0][0] == 0 and sum(n for _, n in spans) == n_total
        for (r0, n0), (r1, _) in zip(spans, spans[1:]):
            assert r0 + n0 == r1


def test_generated_asm_is_up_to_date(tmp_path):
    """The three generated kernel bodies in csrc/ are exactly what tools/gen_mlp_asm.py emits today (no timing-experiment
    switch leaked into them, nobody edited them by hand)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith('NPF16_GEN_')}
    env['NPF16_GEN_OUTDIR'] = str(tmp_path)
    subprocess.run([sys.executable, os.path.join(root, 'tools', 'gen_mlp_asm.py')], check=True, env=env, stdout=subprocess.DEVNULL)
    for name in ('np_mlp_asm.inc', 'np_mlp_asm_dual.inc', 'np_actor_asm.inc', 'np_actor_mfma_asm.inc'):
        with open(tmp_path / name, 'rb') as f, open(os.path.join(root, 'neuralplane_amd', 'csrc', name), 'rb') as g:
            assert f.read() == g.read(), f'{name} is stale: run python tools/gen_mlp_asm.py'


def test_design_kernel_table_is_what_the_library_says():
    """DESIGN.md's "kernels at a glance" block (registers, scratch, LDS per kernel) is generated from the metadata of the code objects inside
    the built library (tools/code_object_table.py) and must not drift from it (the table used to be prose).  Also: every
    generated asm statement that touches vcc declares it, and none ends with a scalar load in flight (the two contracts the parked fault of
    round 3 was suspected of)."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from neuralplane_amd import build
    build.build_hip()
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'code_object_table.py'), '--check-design'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ('np_mlp_asm.inc', 'np_mlp_asm_dual.inc', 'np_actor_mfma16_asm.inc', 'np_actor_mfma_asm.inc', 'np_actor_asm.inc'):
        src = open(os.path.join(root, 'neuralplane_amd', 'csrc', name)).read()
        blocks = re.findall(r'asm volatile\((.*?)\);\n', src, flags=re.S)
        assert blocks, name
        for b in blocks:
            ins = re.findall(r'"([^"\\]*)\\n\\t"', b)
            loads = [i for i, x in enumerate(ins) if x.startswith('s_load') or x.startswith('s_buffer_load')]
            waits = [i for i, x in enumerate(ins) if x.startswith('s_waitcnt') and 'lgkmcnt(0)' in x]
            assert not loads or any(w > loads[-1] for w in waits), f'{name}: a statement ends with a scalar load in flight'
            assert not any('vcc' in x for x in ins) or '"vcc"' in b.split(':')[-1], f'{name}: vcc written but not declared'


def test_env_kernel_instantiations_follow_the_family_rules():
    """The set of f16_env_kernel instantiations in the built library obeys the three family-level rules np_env_tu.inc encodes: the GEMM-order
    bodies are single-set (no pair variant, WPT == 2, with GEMM), the latency family (64-aircraft tiles) is built for Euler only, and per task
    the GEMM family is the non-GEMM family minus the pair variants — so an edit of the dispatch cannot quietly add or drop kernels."""
    import importlib.util
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from neuralplane_amd import build
    spec = importlib.util.spec_from_file_location('_code_object_table', os.path.join(root, 'tools', 'code_object_table.py'))
    cot = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cot)
    val = {'true': True, 'false': False}
    fam = {}   # (task, GEMM) -> {(SOLVER, STEP, CACHED, TILE, WPT, INNER, PW)}
    for row in cot.kernels_of(build.build_hip()):
        m = re.fullmatch(r'npf16::f16_env_kernel<(.*)>', cot.kernel_key(row[0]))
        if not m:
            continue
        args = [val[x] if x in val else int(x) for x in m.group(1).split(', ')]
        assert len(args) == 9, row[0]
        task, solver, step, cached, tile, wpt, inner, pw, gemm = args
        assert not (wpt == 2 and gemm), f'{row[0]}: pair variant with GEMM-order bodies'
        assert not (solver == 1 and tile == 64), f'{row[0]}: rk4 latency kernel'
        variant = (solver, step, cached, tile, wpt, inner, pw)
        assert variant not in fam.setdefault((task, gemm), set()), f'{row[0]}: instantiated twice'
        fam[(task, gemm)].add(variant)
    assert sorted(fam) == [(t, g) for t in range(3) for g in (False, True)]
    for task in range(3):
        assert fam[(task, True)] == {v for v in fam[(task, False)] if v[4] != 2}, f'task {task}: GEMM family != non-GEMM family minus the pair variants'


def test_two_set_phase_statements_by_emulation():
    """The generated pair-variant statements (np_mlp_asm_dual.inc: ~20 000 lines of inline asm) executed as TEXT by
    tools/emulate_dual_asm.py — scalar control flow, weight stream, packed FMAs with op_sel / clamp, LDS traffic — on a synthetic
    blob in the KBLOB_DUAL layout: every net of every phase, both accumulator sets, equals the spec's evaluation; with the scalar
    loads landing at their s_waitcnt and at once (no instruction reads a buffer with a load in flight); every load inside the blob."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('emulate_dual_asm', os.path.join(root, 'tools', 'emulate_dual_asm.py'))
    emu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(emu)
    assert emu.check(land_at_wait=True) == []
    assert emu.check(land_at_wait=False, seed=3) == []
    # the emulator does notice a broken stream: scale the first record of the blob and its coefficient goes wrong
    blob, nets, xa, xb = emu.build_blob(0)
    lines, start = emu.statement(open(emu.INC).read(), 'FORCE2', 0)
    good, loads = emu.run_statement(lines, start, blob, xa, xb, True)
    blob2 = blob.copy()
    blob2[start:start + 288] *= 1.5
    bad, _ = emu.run_statement(lines, start, blob2, xa, xb, True)
    assert any(good[k] != bad[k] for k in good) and min(loads) >= 0


def test_pair_plans_are_balanced_and_complete():
    """tools/gen_mlp_asm.py::PAIR_PLANS (mirrored by np_f16_device.h::PAIR_*, tied by static_asserts in the generated file): the
    two waves of a pair get the same number of VALU instructions within 3 % (4 % in the un-cached phase), and together they cover every net of the phase
    exactly once."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'tools', 'gen_mlp_asm.py')).read().replace("if __name__ == '__main__':", 'if False:')
    g = {'__file__': os.path.join(root, 'tools', 'gen_mlp_asm.py')}
    exec(compile(src, 'gen_mlp_asm', 'exec'), g)
    cost = {shape: sum(1 for i in g['BodyNM'](shape, 0).build() if i.startswith('v_')) for shape in g['SHAPES']}   # the two-set bodies
    classes = {c[0]: c for c in g['CLASSES']}
    for kind, waves in g['PAIR_PLANS'].items():
        loads = [sum(cost[classes[c][1]] * n for c, _, n in w) for w in waves]
        assert abs(loads[0] - loads[1]) <= (0.04 if kind == 'ALL' else 0.03) * max(loads), (kind, loads)   # ALL: the un-cached evaluation, first step only
        want = {(classes_name, k) for ci, first, n in g['phase_items'](kind) for classes_name in [g['CLASSES'][ci][0]] for k in range(first, first + n)}
        got = [(c, k) for w in waves for c, first, n in w for k in range(first, first + n)]
        assert len(got) == len(set(got)) and set(got) == want, kind


def test_bench_self_launch_and_prelude_count(monkeypatch):
    """bench.py without a launcher environment: `--gpus N` re-executes under torch.distributed.run (127.0.0.1, one rank per GPU,
    `--n` spelled `--aircraft` for the launcher's parser); the prelude's step count is a pure function of an estimate that is
    identical on every rank (steps may hold collectives: a time-based count diverges between ranks and deadlocks)."""
    import importlib.util
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(root, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seen = {}
    monkeypatch.setattr(bench.subprocess, 'call', lambda cmd, env=None: seen.update(cmd=cmd, env=env) or 0)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4', '--n', '1000', '--steps', '7'])
    args = type('A', (), {'gpus': 4})()
    assert bench.self_launch(args) == 0
    cmd = seen['cmd']
    assert cmd[1:4] == ['-m', 'torch.distributed.run', '--nnodes=1'] and '--nproc-per-node=4' in cmd
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1' and '--aircraft' in cmd and '--n' not in cmd
    assert seen['env']['HSA_ENABLE_IPC_MODE_LEGACY'] == '0'

    class Dev:
        pass
    calls = []
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda dev=None: None)
    tm = bench.Timer(lambda i: calls.append(i), None, Dev(), None, 'gloo')
    n1, _, nxt = tm.prelude(0.3, i0=5, est_step_s=0.004)
    assert n1 == 75 and nxt == 80 and calls == list(range(5, 80))
    assert tm.prelude(0.0, i0=0, est_step_s=0.004)[0] == 0
    st = bench.stats([0.3, 0.1, 0.2])
    assert st['kernel_median_ms'] == 0.2 and st['kernel_min_ms'] == 0.1 and st['launches_timed'] == 3


# ---------------------------------------------------------------------------------------------------
# the env-side API surface of the reference, name by name (tests/golden/ref_api_surface.json <- tools/gen_api_surface.py)
# ---------------------------------------------------------------------------------------------------
def test_mirror_defines_every_name_of_the_reference_env_surface(golden_dir):
    import importlib
    import json
    ref = json.load(open(f'{golden_dir}/ref_api_surface.json'))
    missing = []
    for rel, surf in ref.items():
        mod = importlib.import_module('neuralplane_amd.' + rel[:-3].replace('/', '.'))
        for cls, methods in surf['classes'].items():
            c = getattr(mod, cls, None)
            if not isinstance(c, type):
                missing.append(f'{rel}: class {cls}')
                continue
            missing += [f'{rel}: {cls}.{m}' for m in methods if not hasattr(c, m)]
        missing += [f'{rel}: {f}()' for f in surf['functions'] if not callable(getattr(mod, f, None))]
    assert not missing, missing
    assert sum(len(v['functions']) + sum(len(m) for m in v['classes'].values()) for v in ref.values()) > 120


def test_geodesy_helpers_against_the_reference(golden_dir):
    from neuralplane_amd.envs.utils import utils as U
    g = np.load(f'{golden_dir}/geodesy_kat.npz')
    rows = range(len(g['lat']))
    ecef = np.array([U.geodetic_to_ecef(g['lat'][i], g['lon'][i], g['h'][i]) for i in rows])
    assert np.abs(ecef - g['ecef']).max() < 1e-6
    enu = np.array([U.ecef_to_enu(*g['ecef'][i], g['lat0'][i], g['lon0'][i], g['h0'][i]) for i in rows])
    assert np.abs(enu - g['enu']).max() < 1e-6
    enu2 = np.array([U.geodetic_to_enu(g['lat'][i], g['lon'][i], g['h'][i], g['lat0'][i], g['lon0'][i], g['h0'][i]) for i in rows])
    assert np.abs(enu2 - g['enu2']).max() < 1e-6
    back = np.array([U.enu_to_ecef(*g['enu_in'][i], g['lat0'][i], g['lon0'][i], g['h0'][i]) for i in rows])
    assert np.abs(back - g['ecef_from_enu']).max() < 1e-6
    for got, key in ((np.array([U.ecef_to_geodetic(*g['ecef'][i]) for i in rows]), 'geo_from_ecef'),
                     (np.array([U.enu_to_geodetic(*g['enu_in'][i], g['lat0'][i], g['lon0'][i], g['h0'][i]) for i in rows]), 'geo_from_enu')):
        assert np.abs(got[:, :2] - g[key][:, :2]).max() < 1e-11 and np.abs(got[:, 2] - g[key][:, 2]).max() < 1e-6
    # the round trip closes, also on the polar axis
    assert np.allclose(U.ecef_to_geodetic(*U.geodetic_to_ecef(47.0, -122.0, 1234.5)), (47.0, -122.0, 1234.5), atol=1e-9)
    assert abs(U.ecef_to_geodetic(0.0, 0.0, 6.4e6)[0] - 90.0) < 1e-12


def test_pairwise_helpers_against_the_reference(golden_dir):
    """get_AO_TA_R ... distance_fn on tensors (utils.py:156-250): the golden vectors the combat oracle is pinned with."""
    from neuralplane_amd.envs.utils import utils as U
    p = np.load(f'{golden_dir}/pairwise_kat.npz')
    T = [torch.from_numpy(p[k]) for k in ('ego_pos', 'enm_pos', 'ego_vel', 'enm_vel')]
    AO, TA, R = U.get_AO_TA_R(*T)
    AO2, TA2, R2, side = U.get2d_AO_TA_R(*T, return_side=True)
    assert len(U.get_AO_TA_R(*T, return_side=True)) == 4 and len(U.get2d_AO_TA_R(*T)) == 3
    Rkm = R * 0.3048 / 1000
    got = dict(AO=AO, TA=TA, R=R, AO2=AO2, TA2=TA2, R2=R2, side=side, orient=U.orientation_reward(AO, TA), range=U.range_reward(3, Rkm),
               ofn=U.orientation_fn(AO), dfn=U.distance_fn(Rkm))
    for k, v in got.items():
        ref = p[k]
        err = np.abs(v.numpy() - ref) / np.maximum(np.abs(ref), 1.0)
        assert np.nanmax(err) < 1e-6, k
        assert np.array_equal(np.isnan(v.numpy()), np.isnan(ref)), k
    for fn, args in ((U.orientation_reward, (AO, TA)), (U.range_reward, (3, Rkm))):
        with pytest.raises(NotImplementedError):
            fn(*args, version='v9')
    for v in ('v0', 'v1'):
        assert torch.isfinite(U.orientation_reward(AO[4:], TA[4:], version=v)).all()
    for v in ('v0', 'v1', 'v2'):
        assert torch.isfinite(U.range_reward(3, Rkm, version=v)).all()


def test_i8_weight_packer_agrees_with_the_oracles_quantiser(golden_dir):
    """np_actor_pack_i8 (the library's load-time packer, host code: runs here without a GPU) against oracle/f16_actor_i8.inc's independent
    quantiser: un-shuffling the fragment order (M-block / k-step / limb / lane / 16 bytes, k-slot e of half h <-> input feature
    32 ks + 8 (e >> 2) + 4 h + (e & 3)) gives the same sign + 29-bit integers, the scales are 2^(ew - 18), k-slots beyond 22 inputs of the
    first layer are zero, the float prefix is the fp32 layout unchanged, the LayerNorm bound constants are max |gamma|, max |beta|."""
    import numpy as np
    from neuralplane_amd.actor import NUM_FLOATS, NUM_FLOATS_I8, pack_i8, pack_ppo_actor
    from oracle.f16_oracle import ActorOracle
    d = np.load(f'{golden_dir}/actor_kat.npz')
    w = pack_ppo_actor({k[4:]: d[k] for k in d.files if k.startswith('sd::')})
    out = pack_i8(w)
    assert out.size == NUM_FLOATS_I8 and np.array_equal(out[:NUM_FLOATS], w)
    o = ActorOracle(w, 'i8')
    frag = out[NUM_FLOATS + 4368:].view(np.uint8)      # after the fp32 prefix and the 4 368 floats of tables
    assert frag.size == 592 * 1024
    sw_off = NUM_FLOATS
    base = 0
    for layer, (n_in, n_out, ks_count) in enumerate(((22, 128, 1), (128, 128, 4), (128, 384, 4), (128, 384, 4), (128, 128, 4), (128, 128, 4))):
        wq, ew = o.quantised_weights(layer)
        blocks = n_out // 32
        f = frag[base: base + blocks * ks_count * 4 * 1024].reshape(blocks, ks_count, 4, 64, 16).astype(np.int64)
        f = np.where(f >= 128, f - 256, f)                                   # signed limb bytes
        val = ((f[:, :, 3] * 256 + f[:, :, 2]) * 256 + f[:, :, 1]) * 256 + f[:, :, 0]     # [mb, ks, lane, e]
        got = np.zeros((n_out, 32 * ks_count), np.int64)
        for ks in range(ks_count):
            for hh in range(2):
                for e in range(16):
                    got[:, 32 * ks + 8 * (e >> 2) + 4 * hh + (e & 3)] = val[:, ks, 32 * hh: 32 * hh + 32, e].reshape(-1)
        assert np.array_equal(got[:, :n_in], wq), layer
        assert not got[:, n_in:].any(), layer
        assert np.array_equal(out[sw_off: sw_off + n_out], np.ldexp(np.float32(1), ew - 18).astype(np.float32)), layer
        sw_off += n_out
        base += blocks * ks_count * 4 * 1024
    lnmax = out[NUM_FLOATS + 4356: NUM_FLOATS + 4356 + 12]
    assert lnmax[0] == np.abs(w[0:22]).max() and lnmax[1] == np.abs(w[22:44]).max()
    tab = out[NUM_FLOATS: NUM_FLOATS + 4368]
    assert np.array_equal(tab[1280: 1280 + 128], w[44: 44 + 128]) and np.array_equal(tab[3840: 3840 + 512], w[NUM_FLOATS - 512:]) and np.array_equal(tab[4352: 4356], w[NUM_FLOATS - 516: NUM_FLOATS - 512])


def _policy_state_dicts(hid=128, gru_layers=1, mlp_layers=2, act_dim=4, obs_dim=22):
    """(actor, critic) state_dicts with the reference's PPOActor / PPOCritic keys for --hidden-size / --act-hidden-size "hid x mlp_layers",
    --recurrent-hidden-size hid, --recurrent-hidden-layers gru_layers (algorithms/utils/mlp.py, gru.py; config.py:48-285)."""
    rng = np.random.RandomState(0)

    def trunk(mlp):
        sd = {'base.feature_norm.weight': np.ones(obs_dim), 'base.feature_norm.bias': np.zeros(obs_dim)}
        for stack, first in (('base.mlp', obs_dim), (mlp, hid)):
            i = first
            for layer in range(mlp_layers):
                sd[f'{stack}.fc.{3 * layer}.weight'], sd[f'{stack}.fc.{3 * layer}.bias'] = rng.normal(size=(hid, i)), np.zeros(hid)
                sd[f'{stack}.fc.{3 * layer + 2}.weight'], sd[f'{stack}.fc.{3 * layer + 2}.bias'] = np.ones(hid), np.zeros(hid)
                i = hid
        for layer in range(gru_layers):
            for k in ('ih', 'hh'):
                sd[f'rnn.gru.weight_{k}_l{layer}'], sd[f'rnn.gru.bias_{k}_l{layer}'] = rng.normal(size=(3 * hid, hid)), np.zeros(3 * hid)
        sd['rnn.norm.weight'], sd['rnn.norm.bias'] = np.ones(hid), np.zeros(hid)
        return sd
    a, c = trunk('act.mlp'), trunk('mlp')
    a['act.action_out.mu_net.fc.0.weight'], a['act.action_out.mu_net.fc.0.bias'], a['act.action_out.log_std'] = rng.normal(size=(act_dim, hid)), np.zeros(act_dim), np.zeros(act_dim)
    c['value_out.weight'], c['value_out.bias'] = rng.normal(size=(1, hid)), np.zeros(1)
    return ({k: np.asarray(v, np.float32) for k, v in a.items()}, {k: np.asarray(v, np.float32) for k, v in c.items()})


@pytest.mark.parametrize('kw', [dict(hid=64), dict(hid=256), dict(gru_layers=2), dict(mlp_layers=3)])
def test_fused_policy_packers_name_the_supported_shape_for_any_other(kw):
    """the reference takes --hidden-size / --act-hidden-size / --recurrent-hidden-size / --recurrent-hidden-layers from the
    command line (/root/reference/config.py:48-285); the fused kernels exist for one shape.  Any other must be a ValueError that names the
    supported one (FusedPolicy / FusedActor construct through these packers), never a silently mis-packed network."""
    from neuralplane_amd.actor import pack_ppo_actor
    from neuralplane_amd.policy import pack_policy_actor, pack_policy_critic
    sa, sc = _policy_state_dicts(**kw)
    for pack, sd in ((pack_policy_actor, sa), (pack_policy_critic, sc), (pack_ppo_actor, sa)):
        with pytest.raises(ValueError, match='128'):
            pack(sd)
    sa, sc = _policy_state_dicts()
    assert pack_policy_actor(sa)[0].size == pack_policy_critic(sc).size == pack_ppo_actor(sa).size == 153392


def test_bench_contract_line_is_small_and_complete():
    """bench.py's LAST stdout line is what the driver parses: built from the full record by contract_line(), it must stay under 4 KB whatever
    the details hold (round 5: one 28.8 KB line, `parsed: null`), carry the contract fields, and refuse to grow."""
    import json
    import bench
    big = {'note': 'x' * 30000}
    out = {'metric': bench.METRIC, 'value': 3.6e9, 'unit': 'aircraft-steps/s', 'n_gpus': 1, 'steps': 20, 'warmup': 5, 'ms_per_step': 0.27,
           'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
           'config': {'workload': 'F-16 heading, N=1000000', 'aircraft_per_gpu': 1000000, 'sharding': 'rows', 'other': big},
           'roofline': {'bound': 'valu', 'achieved': 124.0, 'peak': 157.3, 'unit': 'TFLOP/s', 'frac': 0.79, 'executed_frac': 0.6, 'kernel': 'k',
                        'kernel_avg_ms': 0.27, 'traffic': 4.0e8, 'traffic_source': 'profiles/x.json', 'algorithmic_bytes_per_launch': 2.78e8, 'note': 'y' * 5000},
           'roofline_hbm': {'achieved': 1000.0, 'frac': 0.125},
           'cpu_baseline': {'value': 1.1e6, 'unit': 'aircraft-steps/s', 'cores': 16, 'kind': 'port', 'sample': 's', 'torch_eager': {'value': 2e5, 'note': 'z' * 3000},
                            'reference_context': big},
           'optional_modes': big, 'cold_start': big, 'per_rank': big, 'expected_scaling': big, 'world_size': 1, 'backend': None, 'state_finite': True}
    txt = bench.contract_line(out, 'gpurun_out/bench_details.json')
    line = json.loads(txt)
    assert len(txt) < 4000 and '\n' not in txt
    assert line['value'] == 3.6e9 and line['roofline']['frac'] == 0.79 and line['cpu_baseline']['value'] == 1.1e6 and line['cpu_baseline']['torch_eager'] == 2e5
    assert 'optional_modes' not in line and 'note' not in line['roofline'] and set(line['config']) == {'workload', 'aircraft_per_gpu', 'sharding'}
    out['config']['workload'] = 'w' * 5000
    with pytest.raises(SystemExit):
        bench.contract_line(out)


def test_i8_weight_packer_reports_its_errors_through_the_library():
    """np_actor_pack_i8 used to return 1 without setting the error string (a stale message surfaced) and pushed NaN / infinite
    weights through (int32_t)nearbyint(...): undefined behaviour.  Both are library errors with their own message now."""
    from neuralplane_amd.actor import NUM_FLOATS, pack_i8
    w = np.random.RandomState(0).normal(0, 0.05, NUM_FLOATS).astype(np.float32)
    assert pack_i8(w).size == 309312
    for bad in (np.nan, np.inf):
        w2 = w.copy()
        w2[1234] = bad
        with pytest.raises(RuntimeError, match='non-finite weight'):
            pack_i8(w2)


def test_airframe_block_defaults_and_validation():
    """np_f16_airframe (ABI 16): np_f16_airframe_default() writes the reference's literals (F16_dynamics.py:61-76,114-116, 22-35; F16_model.py:52-62);
    `_lib.airframe({})` is the all-zero block (= the F-16); unknown fields are refused on the Python side."""
    from neuralplane_amd import _lib
    a = _lib.airframe({'mass': 700.0})
    assert (a.g, a.mass, a.B, a.S, a.cbar, a.xcgr, a.xcg, a.Heng) == (32.17, 700.0, 30.0, 300.0, 11.32, 0.35, 0.30, 0.0)
    assert (a.Jy, a.Jxz, a.Jz, a.Jx, a.ail_ref, a.rud_ref) == (55814.0, 982.0, 63100.0, 9496.0, 21.5, 30.0)
    assert (a.atm_lapse, a.atm_exp, a.rho0, a.lag_keep, a.lag_new, a.thrust_frac, a.thrust_max, a.thrust_unit) == (0.703e-5, 4.14, 2.377e-3, 0.9, 0.1, 0.225, 76300.0, 0.3048)
    assert list(a.surf_max) == [45.0, 45.0, 45.0]
    z = _lib.airframe(None)
    assert bytes(z) == bytes(len(bytes(z)))
    with pytest.raises(ValueError, match='unknown field'):
        _lib.airframe({'wingspan': 30})
    cfg = parse_config('heading')
    cfg.airframe = {'Jy': 60000.0}
    c = cfg_from_config(cfg, 'heading')
    assert c.airframe.Jy == 60000.0 and c.airframe.mass == 636.94
    assert bytes(cfg_from_config(parse_config('heading'), 'heading').airframe) == bytes(z)


def test_ctx_create_refuses_an_unphysical_airframe_before_it_touches_a_device():
    import ctypes as C
    from neuralplane_amd import _lib
    from neuralplane_amd.core import ASSET_BLOB
    lib = _lib.load()
    blob = open(ASSET_BLOB, 'rb').read()
    for bad, msg in (({'mass': -1.0}, 'positive'), ({'Jxz': 1e6}, 'Jx Jz - Jxz'), ({'atm_exp': 0.0}, 'positive'), ({'g': float('nan')}, 'non-finite')):
        cfg = parse_config('heading')
        cfg.airframe = bad
        c = cfg_from_config(cfg, 'heading')
        ctx = C.c_void_p()
        assert lib.np_f16_ctx_create(blob, len(blob), C.byref(c), 0, C.byref(ctx)) != 0 and not ctx.value
        assert msg in lib.np_last_error().decode(), lib.np_last_error()
