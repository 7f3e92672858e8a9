"""SyntheticRolloutProblem: the VecGymNE-equivalent over the offline
synthetic environment — the flagship benchmark problem.

Reference parity: the role of VecGymNE
(/root/reference/src/evotorch/neuroevolution/vecgymne.py:95-1073) — a
whole-population batched rollout with on-device observation normalization —
with the env replaced by `SyntheticEnvSpec` (no simulator exists offline)
and the rollout executed by the fused gfx950 kernel
(evotorch_amd/ops/hip/rollout.hip) in ONE launch per generation.
"""

from typing import Optional

import torch

from ..core import Problem, SolutionBatch
from ..ops import seed_from_generator
from .runningnorm import ObsNormLayer, RunningNorm
from .synthetic_env import SyntheticEnvSpec, rollout_eager

__all__ = ["SyntheticRolloutProblem"]


class SyntheticRolloutProblem(Problem):
    _NOT_CLONED = Problem._NOT_CLONED + ("_env_blob_state",)

    def __init__(
        self,
        *,
        spec: Optional[SyntheticEnvSpec] = None,
        device="cpu",
        seed: Optional[int] = None,
        observation_normalization: bool = True,
        decrease_rewards_by: float = 0.0,
        **spec_kwargs,
    ):
        if spec is None:
            spec = SyntheticEnvSpec(device=device, **spec_kwargs)
        self._spec = spec
        super().__init__(
            objective_sense="max",
            solution_length=spec.solution_length,
            initial_bounds=(-0.01, 0.01),
            dtype=torch.float32,
            device=device,
            seed=seed,
            store_solution_stats=False,
        )
        self._obs_norm_enabled = bool(observation_normalization)
        self._obs_norm = RunningNorm(shape=spec.obs_dim, device=device)
        self._decrease_rewards_by = float(decrease_rewards_by)
        self._pending_stats = None
        self._graph_seed_buf: Optional[torch.Tensor] = None  # device seed chain, set by enable_graph_mode
        self._last_interactions = 0
        self._total_interactions = 0
        # Terminating rollouts on the GPU count their interactions on the
        # device, in place in this persistent int64 pair (last evaluation,
        # total), so that replays of a captured generation keep counting.
        # They become host integers only when read.
        self._device_interactions: Optional[torch.Tensor] = None
        self._last_interactions_on_device = False
        self._last_episode_lengths = None  # tensor, or (n, device) after fixed-length episodes
        self._episode_count = 0
        self.after_eval_hook.append(self._after_eval_status_getter)

    # -- properties ----------------------------------------------------------

    @property
    def spec(self) -> SyntheticEnvSpec:
        return self._spec

    @property
    def obs_norm(self) -> RunningNorm:
        return self._obs_norm

    @property
    def last_episode_lengths(self) -> Optional[torch.Tensor]:
        """Steps each member of the last evaluated batch ran, as int32 of
        shape [n] on the problem's device; None before the first
        evaluation."""
        lengths = self._last_episode_lengths
        if isinstance(lengths, tuple):  # fixed-length episodes
            n, device = lengths
            lengths = torch.full((n,), self._spec.episode_length, dtype=torch.int32, device=device)
            self._last_episode_lengths = lengths
        return lengths

    @property
    def last_eval_interaction_count(self) -> int:
        """Environment steps of the last evaluation. After a terminating
        rollout on the GPU, reading this synchronises with the device."""
        if self._last_interactions_on_device:
            return int(self._device_interactions[0])
        return self._last_interactions

    @last_eval_interaction_count.setter
    def last_eval_interaction_count(self, value: int):
        self._last_interactions = int(value)
        self._last_interactions_on_device = False

    @property
    def total_interaction_count(self) -> int:
        """Environment steps of all evaluations so far (one device read
        when terminating rollouts ran on the GPU)."""
        total = self._total_interactions
        if self._device_interactions is not None:
            total += int(self._device_interactions[1])
        return total

    def _norm_mean_std(self):
        if self._obs_norm_enabled and self._obs_norm.has_data:
            return self._obs_norm.mean, self._obs_norm.stdev
        return self._default_mean_std(self._device)

    def _packed_env_blob(self, values: torch.Tensor) -> torch.Tensor:
        """The rollout kernel's env blob with this generation's (mean, std)
        in its tail. The blob is built once per device and lives as long as
        the problem; each evaluation recomputes mean and stdev from the
        running sums straight into its tail in ONE launch
        (ops.obsnorm_pack_), so `obs_norm.update()` / `reset()` between
        generations are seen. It is overwritten in place: the rollout that
        reads it is queued on the same stream before the next pack, and
        nothing else keeps a reference. Without the fused tail the blob is
        concatenated anew from RunningNorm's properties."""
        from .. import ops

        spec = self._spec
        tracked = self._obs_norm_enabled and self._obs_norm.has_data
        device = values.device
        if ops.fused_tail_for(values) is not None:
            state = getattr(self, "_env_blob_state", None)
            if state is None or state[0].device != device:
                # a fresh blob carries the no-data defaults (mean 0, std 1)
                state = [spec.env_blob(*self._default_mean_std(device), device=device), True]
                self._env_blob_state = state
            blob, holds_defaults = state
            O = spec.obs_dim
            if not tracked:
                if not holds_defaults:
                    blob[-2 * O : -O].zero_()
                    blob[-O:].fill_(1.0)
                    state[1] = True
                return blob
            rn = self._obs_norm
            if ops.obsnorm_pack_(blob, blob.numel() - 2 * O, rn._count, rn._sum, rn._sum_sq, rn.min_variance):
                state[1] = False
                return blob
        mean, std = self._norm_mean_std()
        return spec.env_blob(mean, std, device=device)

    def _default_mean_std(self, device):
        O = self._spec.obs_dim
        return (
            torch.zeros(O, dtype=torch.float32, device=device),
            torch.ones(O, dtype=torch.float32, device=device),
        )

    def observation_normalization_data(self):
        mean, std = self._norm_mean_std()
        return {"mean": mean.cpu(), "stdev": std.cpu(), "count": self._obs_norm.count}

    # -- evaluation ----------------------------------------------------------

    def enable_graph_mode(self) -> None:
        """Switch episode seeding to a DEVICE splitmix64 chain so that
        `_evaluate_batch` is hipGraph-capturable (a host-derived seed
        would be frozen into the capture and every replay would rerun the
        same episodes). Called by GraphedSearch; the chain starts from
        the problem's own generator."""
        if self._device.type != "cuda":
            return
        if self._graph_seed_buf is None:
            seed0 = seed_from_generator(self._generator, self._device)
            self._graph_seed_buf = torch.tensor([seed0], dtype=torch.int64, device=self._device)

    def _evaluate_batch(self, batch: SolutionBatch):
        values = batch.access_values(keep_evals=True)
        n = len(batch)
        spec = self._spec
        seed_buf = self._graph_seed_buf
        init_seed = 0 if seed_buf is not None else seed_from_generator(self._generator, self._device) & 0x7FFFFFFF
        member_offset = 0
        comm = self._comm
        if comm is not None and comm.world_size > 1:
            # distinct episode-init streams per rank-sharded member; the
            # per-rank init_seed difference is environment stochasticity
            member_offset = comm.rank * n
        if values.device.type == "cuda":
            from .. import ops

            mod = ops.hip_required()
            blob = self._packed_env_blob(values)
            obs_stats = torch.zeros(2 * spec.obs_dim, dtype=torch.float32, device=values.device)
            if seed_buf is not None:
                mod.bump_seed(seed_buf)  # fresh episode seed per replay, on device
            if spec.terminates:
                lengths = torch.empty(n, dtype=torch.int32, device=values.device)
                fitness = mod.rollout_terminating(
                    values.contiguous(),
                    blob,
                    obs_stats,
                    lengths,
                    spec.obs_dim,
                    spec.act_dim,
                    spec.rank,
                    spec.episode_length,
                    spec.alive_bonus,
                    spec.act_cost,
                    init_seed,
                    member_offset,
                    spec.policy_hidden,
                    spec.health_index,
                    spec.healthy_range[0],
                    spec.healthy_range[1],
                    seed_buf,
                )
                count = lengths.sum()  # stays on the device: no host sync, capturable
            else:
                fitness = mod.rollout_linear(
                    values.contiguous(),
                    blob,
                    obs_stats,
                    spec.obs_dim,
                    spec.act_dim,
                    spec.rank,
                    spec.episode_length,
                    spec.alive_bonus,
                    spec.act_cost,
                    init_seed,
                    member_offset,
                    spec.policy_hidden,
                    seed_buf,
                )
                lengths = None
                count = float(n) * spec.episode_length
            triple = (count, obs_stats[: spec.obs_dim], obs_stats[spec.obs_dim :])
        else:
            mean, std = self._norm_mean_std()
            fitness, triple, lengths = rollout_eager(
                spec,
                values.to(torch.float32),
                mean,
                std,
                init_seed=init_seed,
                member_offset=member_offset,
                return_steps=True,
            )
            lengths = lengths.to(torch.int32) if spec.terminates else None
        if self._decrease_rewards_by != 0.0:
            # per step survived
            survived = spec.episode_length if lengths is None else lengths.to(fitness.dtype)
            fitness = fitness - self._decrease_rewards_by * survived
        batch.set_evals(fitness.to(self._eval_dtype))
        if lengths is None:
            self._last_episode_lengths = (n, values.device)  # all episode_length: built when read
            self.last_eval_interaction_count = n * spec.episode_length
            self._total_interactions += n * spec.episode_length
        elif lengths.device.type == "cuda":
            self._last_episode_lengths = lengths
            counters = self._device_interactions
            if counters is None or counters.device != lengths.device:
                carried = 0 if counters is None else int(counters[1])
                counters = torch.tensor([0, carried], dtype=torch.int64, device=lengths.device)
                self._device_interactions = counters
            counters[0].copy_(triple[0])
            counters[1].add_(triple[0])
            self._last_interactions_on_device = True
            # the count RunningNorm's merge kernel reads on the device
            triple = (triple[0].to(torch.float64).reshape(1), triple[1], triple[2])
        else:
            self._last_episode_lengths = lengths
            self.last_eval_interaction_count = int(triple[0])
            self._total_interactions += int(triple[0])
        self._pending_stats = triple
        self._episode_count += n

    def _after_eval_status_getter(self, batch) -> dict:
        self._merge_pending_stats()
        total = self._total_interactions
        if self._device_interactions is not None:
            # a 0-dim device tensor, like `mean_eval`: no host sync here
            total = self._device_interactions[1] + total
        return {
            "total_interaction_count": total,
            "total_episode_count": self._episode_count,
        }

    def _merge_pending_stats(self):
        """Fold the rollout's (count, Σ, Σ²) into the running norm — with an
        attached Comm this is ONE all-reduce across ranks (P5), and during a
        sharded gradient generation it is FUSED into the gradient all-reduce
        (Problem.request_fused_reduce) so a generation costs exactly two
        collectives: fitness all-gather + fused all-reduce."""
        if self._pending_stats is None or not self._obs_norm_enabled:
            self._pending_stats = None
            return
        count, s, ss = self._pending_stats
        self._pending_stats = None
        comm = self._comm
        if comm is not None and comm.world_size > 1:
            if isinstance(count, torch.Tensor):  # a device count stays there: no .item()
                head = count.reshape(1).to(s.device, torch.float32)
            else:
                head = torch.tensor([count], dtype=torch.float32, device=s.device)
            packed = torch.cat([head, s.reshape(-1), ss.reshape(-1)])
            O = self._spec.obs_dim

            def merge(reduced: torch.Tensor):
                # count stays a device tensor: no host sync
                self._obs_norm.update((reduced[0], reduced[1 : 1 + O], reduced[1 + O :]))

            self.request_fused_reduce(packed, merge)
        else:
            self._obs_norm.update((count, s, ss))

    # -- policy export -------------------------------------------------------

    def to_policy(self, x: torch.Tensor) -> torch.nn.Module:
        spec = self._spec
        O, A, H = spec.obs_dim, spec.act_dim, spec.policy_hidden
        x = torch.as_tensor(x, dtype=torch.float32).detach().cpu().reshape(-1)
        mean, std = self._norm_mean_std()
        layers = []
        if self._obs_norm_enabled:
            layers.append(ObsNormLayer(mean.cpu(), std.cpu()))
        with torch.no_grad():
            if H > 0:
                l1 = torch.nn.Linear(O, H)
                l2 = torch.nn.Linear(H, A)
                off = 0
                l1.weight.copy_(x[off : off + H * O].reshape(H, O)); off += H * O
                l1.bias.copy_(x[off : off + H]); off += H
                l2.weight.copy_(x[off : off + A * H].reshape(A, H)); off += A * H
                l2.bias.copy_(x[off:])
                layers += [l1, torch.nn.Tanh(), l2, torch.nn.Hardtanh()]
            else:
                linear = torch.nn.Linear(O, A)
                linear.weight.copy_(x[: A * O].reshape(A, O))
                linear.bias.copy_(x[A * O :])
                layers += [linear, torch.nn.Hardtanh()]
        policy = torch.nn.Sequential(*layers)
        policy.requires_grad_(False)  # inference artifact
        return policy
