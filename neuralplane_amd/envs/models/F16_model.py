"""F16Model — the reference's model object (envs/models/F16_model.py) backed by SoA device buffers.

The numbers live in `F16Batch` (neuralplane_amd/core.py); `s`/`u` are `[n,12]`/`[n,5]` transposed
VIEWS of the SoA buffers, so `model.s[:, 2]` is a contiguous row and in-place writes by callers
(`model.s[mask] = ...`, planning_env.py:166) land in the buffers the kernels read.  Getters that
need the dynamics (acceleration, load factors, EAS, ...) come from ONE np_f16_derived launch per
state version.  The FDM step itself is not here: it is fused into BaseEnv.step's single kernel.
"""
import torch

from .F16.F16_dynamics import F16Dynamics
from .model_base import BaseModel


class F16Model(BaseModel):
    def __init__(self, config, n, device, random_seed, batch):
        super().__init__(config, n, device, random_seed)
        self._b = batch
        self.num_states = getattr(config, 'num_states', 12)
        self.num_controls = getattr(config, 'num_controls', 5)
        self.dt = getattr(config, 'dt', 0.02)
        self.solver = getattr(config, 'solver', 'euler')
        self.airspeed = getattr(config, 'airspeed', 0)
        self.max_altitude = getattr(config, 'max_altitude', 20000)
        self.min_altitude = getattr(config, 'min_altitude', 19000)
        self.max_vt = getattr(config, 'max_vt', 1200)
        self.min_vt = getattr(config, 'min_vt', 1000)
        self.init_state = config.init_state
        self.recent_s = None
        self.recent_u = None
        self.dynamics = F16Dynamics(batch)          # F16_model.py:20; `dynamics.hifi_F16` is the surrogate object (F16_dynamics.py:13)
        self.hifi_F16 = self.dynamics.hifi_F16

    # state / control as the reference lays them out ([n,k]); views, not copies
    @property
    def s(self):
        return self._b.s.t()

    @s.setter
    def s(self, value):
        self._b.s.copy_(torch.as_tensor(value, device=self._b.device).t())

    @property
    def u(self):
        return self._b.u.t()

    @u.setter
    def u(self, value):
        self._b.u.copy_(torch.as_tensor(value, device=self._b.device).t())

    def reset(self, env):
        """F16Model.reset(env) (reference F16_model.py:33-45): state and controls of the rows `env` has flagged (is_done | bad_done |
        exceed_time_limit) are re-initialised — one launch of the reset kernel on the env's flags; targets, step counters and the flags
        themselves stay (BaseEnv.reset() is the call that also runs task.reset and clears them, in the same single launch)."""
        if env is not None and getattr(env, '_batch', None) is not self._b:
            raise ValueError('F16Model.reset(env): env must be the env this model belongs to')
        self._b.model_reset()
        self.recent_s, self.recent_u = None, None      # (the reference copies s / u of the reset rows into recent_*: see update)

    def update(self, action):
        """F16Model.update(action) (reference F16_model.py:51-67): clamp, first-order control lag, one integrator step — ONE kernel launch
        (np_f16_io.inner_step = NP_INNER_UPDATE_ONLY), for callers that drive the model directly as envs/planning_env.py:160 and
        example/quick_start.ipynb do.  `recent_s` / `recent_u` hold the state / controls from before the call, as the reference's do
        ([n, 12] / [n, 5] copies: the one thing here that is not free — BaseEnv.step does not keep them)."""
        self.recent_s, self.recent_u = self.s.clone(), self.u.clone()
        self._b.update(torch.as_tensor(action, device=self._b.device))

    def rollout(self, actions, s=None, u=None, fanout=1, record_every=0, shape='auto', horizon=None):
        """Open-loop look-ahead: `for t in range(H): update(actions[t])` on a copy of the state, as ONE kernel launch (F16Batch.rollout,
        np_f16_model_rollout) — bit-identical to H update() calls, and this model's s / u / recent_* are left exactly as they were.
        actions [H, n * fanout, >=4] (or [n * fanout, >=4] with horizon=H: one held action); s [n0, 12] / u [n0, 5] default to the current
        state; output row r starts from row r // fanout.  Returns (s_end [n * fanout, 12], u_end [n * fanout, 5][, s_traj [H // k, n * fanout, 12]])
        in this class's row-major layout (views)."""
        if s is not None:
            s = torch.as_tensor(s, device=self._b.device).t()
        if u is not None:
            u = torch.as_tensor(u, device=self._b.device).t()
        out = self._b.rollout(actions, s, u, fanout=fanout, record_every=record_every, shape=shape, horizon=horizon)
        return (out[0].t(), out[1].t()) + ((out[2].transpose(1, 2),) if len(out) > 2 else ())

    def rollout_diff(self, actions, s=None, u=None, fanout=1, horizon=None):
        """rollout(record_every=1) that loss.backward() works through (F16Batch.rollout_diff: the backward pass is ONE launch,
        np_f16_model_rollout_vjp; Euler only): differentiable with respect to actions, s [n0, 12] and u [n0, 5].
        Returns (s_traj [H, n * fanout, 12], u_end [n * fanout, 5]) in this class's row-major layout (views)."""
        if s is not None:
            s = torch.as_tensor(s, device=self._b.device).t()
        if u is not None:
            u = torch.as_tensor(u, device=self._b.device).t()
        s_traj, u_end = self._b.rollout_diff(actions, s, u, fanout=fanout, horizon=horizon)
        return s_traj.transpose(1, 2), u_end.t()

    def ilqr_backward(self, actions, s_traj, g_s_traj, g_actions, h_s, h_a, mu, g_u_end=None, s=None, u=None, fanout=1, want_value=False):
        """iLQR's backward pass about rollout(actions, record_every=1) as ONE kernel launch (F16Batch.ilqr_backward,
        np_f16_model_ilqr_backward; Euler only), in this class's row-major layout: s_traj / g_s_traj [H, n * fanout, 12], g_actions
        [H, n * fanout, 4], g_u_end [n * fanout, 4], s [n0, 12], u [n0, 5]; h_s [H, 12], h_a [4] and mu as there.
        Returns (k [H, n * fanout, 4], K [H, n * fanout, 4, 16], dV [n * fanout, 2], status [n * fanout][, p0 [n * fanout, 16],
        P0 [n * fanout, 16, 16]]) — strided views of the planar buffers."""
        t = lambda x: None if x is None else torch.as_tensor(x, device=self._b.device).transpose(-1, -2)  # noqa: E731
        out = self._b.ilqr_backward(actions, t(s_traj), t(g_s_traj), t(g_actions), h_s, h_a, mu, g_u_end=t(g_u_end), s=t(s), u=t(u), fanout=fanout,
                                    want_value=want_value)
        k, K, dV, status = out[:4]
        res = (k.transpose(1, 2), K.permute(0, 3, 1, 2), dV.t(), status)
        return res + ((out[4].t(), out[5].permute(2, 0, 1)) if want_value else ())

    def ilqr_forward(self, actions, s_traj, k, K, alphas, s=None, u=None, fanout=1, s_init=None, u_init=None, cost=None, shape='auto', want_best=True):
        """iLQR's forward pass — the feedback rollout under ilqr_backward's gains for every step size of `alphas` — as ONE kernel launch
        (F16Batch.ilqr_forward, np_f16_model_rollout_feedback; Euler only), in this class's row-major layout: s_traj [H, P, 12], k [H, P, 4],
        K [H, P, 4, 16], s [n0, 12], u [n0, 5], s_init [P, 12], u_init [P, 5], cost = (h_s [H, 12], h_a [4], s_ref [H, P, 12]).
        Returns (actions_new [H, P * L, 4], s_end [P * L, 12], u_end [P * L, 5], s_traj_new [H, P * L, 12][, cost [P * L][, best [P]]]) —
        strided views of the planar buffers; row r is problem r // L with step size alphas[r % L]."""
        t = lambda x: None if x is None else torch.as_tensor(x, device=self._b.device).transpose(-1, -2)  # noqa: E731
        if cost is not None:
            cost = (cost[0], cost[1], t(cost[2]))
        out = self._b.ilqr_forward(actions, t(s_traj), t(k), torch.as_tensor(K, device=self._b.device).permute(0, 2, 3, 1), alphas, s=t(s), u=t(u),
                                   fanout=fanout, s_init=t(s_init), u_init=t(u_init), cost=cost, shape=shape, want_best=want_best)
        return (out[0], out[1].t(), out[2].t(), out[3].transpose(1, 2)) + out[4:]

    def mppi(self, actions, sigma, temperature, cost, candidates, s=None, u=None, seed=None, call0=None, hold=1, shape='auto', want_candidates=False):
        """One MPPI iteration — sample K candidates around the plan, fly them, cost them, re-weight — as ONE library call (F16Batch.mppi,
        np_f16_model_mppi; Euler only), in this class's row-major layout: actions [H, P, >=4], s [P, 12], u [P, 5],
        cost = (h_s [H, 12], h_a [4], s_ref [H, P, 12]).  This model's s / u / recent_* and the env's random stream are left as they were.
        Returns (plan [H, P, 4], cost [P * K], best [P], ess [P][, candidates [H, P * K, 4]])."""
        t = lambda x: None if x is None else torch.as_tensor(x, device=self._b.device).transpose(-1, -2)  # noqa: E731
        return self._b.mppi(actions, sigma, temperature, (cost[0], cost[1], t(cost[2])), candidates, s=t(s), u=t(u), seed=seed, call0=call0, hold=hold,
                            shape=shape, want_candidates=want_candidates)

    def linearize(self, s=None, u=None, want_xdot=True):
        """xdot = f(s, u), A = df/ds, B = df/du of the flight dynamics about a flight condition, per aircraft, as ONE kernel launch
        (F16Batch.linearize, np_f16_model_linearize): what trim solvers, LQR / gain scheduling, iLQR and stability analysis start from.
        s [n0, 12] / u [n0, 5] default to the current state; this model's s / u / recent_* are left exactly as they were.
        Returns (xdot [n0, 12] or None, A [n0, 12, 12], B [n0, 12, 4]) — strided views of the planar buffers: the results are not copied.
        With s and u omitted no torch kernel runs; a given s / u [n0, k] is transposed into the planar layout first (one torch copy each)."""
        if s is not None:
            s = torch.as_tensor(s, device=self._b.device).t()
        if u is not None:
            u = torch.as_tensor(u, device=self._b.device).t()
        xdot, A, B = self._b.linearize(s, u, want_xdot=want_xdot)
        return (xdot.t() if xdot is not None else None), A.permute(2, 0, 1), B.permute(2, 0, 1)

    def trim(self, s, u, unknowns, rows, target=None, **kw):
        """Batched trim — a damped Newton solve per aircraft for a steady flight condition, run to convergence in ONE kernel launch
        (F16Batch.trim, np_f16_model_trim; core.trim_problem builds unknowns / rows / scale / lo / hi), in this class's row-major layout:
        s [n0, 12], u [n0, 5], target [n0, 12].  This model's s / u / recent_* are left exactly as they were.
        Returns (s [n0, 12], u [n0, 5], res [n0], iters [n0], status [n0][, xdot [n0, 12], A [n0, 12, 12], B [n0, 12, 4]]) — views."""
        t = lambda x: None if x is None else torch.as_tensor(x, device=self._b.device).t()  # noqa: E731
        out = self._b.trim(t(s), t(u), unknowns, rows, target=t(target), **kw)
        return (out[0].t(), out[1].t()) + out[2:5] + ((out[5].t(), out[6].permute(2, 0, 1), out[7].permute(2, 0, 1)) if len(out) > 5 else ())

    def lqr(self, A, B, h_s, h_a, **kw):
        """Batched LQR — the steady-state gain of the update() step map at each operating point's (A, B), the discrete algebraic Riccati
        equation solved by structured doubling in ONE kernel launch (F16Batch.lqr, np_f16_model_lqr), in this class's row-major layout:
        A [n0, 12, 12], B [n0, 12, 4] as linearize / trim return them.  This model's s / u / recent_* are left exactly as they were.
        Returns (K [n0, 4, 16], doublings [n0], res [n0], status [n0][, P [n0, 16, 16] with want_P=True]) — views."""
        dev = self._b.device
        out = self._b.lqr(torch.as_tensor(A, device=dev).permute(1, 2, 0), torch.as_tensor(B, device=dev).permute(1, 2, 0), h_s, h_a, **kw)
        return (out[0].permute(2, 0, 1),) + out[1:4] + tuple(x.permute(2, 0, 1) for x in out[4:])

    def ekf(self, actions, z, P, q, r, measure, s=None, u=None, **kw):
        """Batched extended Kalman filter — H predict + update steps of update() per aircraft in ONE kernel launch (F16Batch.ekf,
        np_f16_model_ekf; Euler only), in this class's row-major layout: actions [H, n0, >=4], z [H, n0, 16] (NaN = a missing sample),
        P [n0, 16, 16], s [n0, 12], u [n0, 5] (default: the current state).  This model's s / u / recent_* are left exactly as they were.
        Returns (s [n0, 12], u [n0, 5], P [n0, 16, 16], status [n0][, x_traj [H, n0, 16], pdiag_traj [H, n0, 16], nis [H, n0] with
        want_traj=True]) — views."""
        t = lambda x: None if x is None else torch.as_tensor(x, device=self._b.device).transpose(-1, -2)  # noqa: E731
        out = self._b.ekf(actions, t(z), torch.as_tensor(P, device=self._b.device).permute(1, 2, 0), q, r, measure, s=t(s), u=t(u), **kw)
        return (out[0].t(), out[1].t(), out[2].permute(2, 0, 1), out[3]) + tuple(x.transpose(1, 2) for x in out[4:6]) + out[6:]

    def get_extended_state(self):
        """nlplant(hstack(s,u)) — reference returns [n,17] with zero control derivatives (F16_model.py:47-49)."""
        d = self._b.derived()
        out = torch.zeros((self.n, 17), dtype=torch.float32, device=self._b.device)
        out[:, :12] = d[0:12].t()
        return out

    def get_state(self):
        return self.s

    def get_control(self):
        return self.u

    def get_position(self):
        b = self._b.s
        return b[0], b[1], b[2]

    def get_ground_speed(self):
        d = self._b.derived()
        return d[0], d[1]

    def get_climb_rate(self):
        return self._b.derived()[2]

    def get_posture(self):
        b = self._b.s
        return b[3], b[4], b[5]

    def get_euler_angular_velocity(self):
        d = self._b.derived()
        return d[3], d[4], d[5]

    def get_vt(self):
        return self._b.s[6]

    def get_TAS(self):
        return self._b.s[6] + self.airspeed * torch.ones_like(self._b.s[6])

    def get_EAS(self):
        return self._b.derived()[19]

    def get_AOA(self):
        return self._b.s[7]

    def get_AOS(self):
        return self._b.s[8]

    def get_angular_velocity(self):
        b = self._b.s
        return b[9], b[10], b[11]

    def get_thrust(self):
        return self._b.u[0]

    def get_control_surface(self):
        u = self._b.u
        return u[1], u[2], u[3], u[4]

    def get_velocity(self):
        s = self._b.s
        sina, cosa, sinb, cosb = torch.sin(s[7]), torch.cos(s[7]), torch.sin(s[8]), torch.cos(s[8])
        return s[6] * cosb * cosa, s[6] * sinb, s[6] * cosb * sina

    def get_acceleration(self):
        d = self._b.derived()
        return d[12], d[13], d[14]

    def get_accels(self):
        d = self._b.derived()
        return d[15], d[16], d[17]

    def get_G(self):
        nx, ny, nz = self.get_accels()
        return torch.sqrt(nx ** 2 + ny ** 2 + nz ** 2)

    def get_EAS2TAS(self):
        return self._b.derived()[18]

    def get_atmos(self):
        """(mach, qbar, ps) — F16_model.py:183-198."""
        d = self._b.derived()
        return d[20], d[21], d[22]
