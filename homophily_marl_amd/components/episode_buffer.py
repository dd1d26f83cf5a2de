"""Episode storage with the reference's surface (src/components/episode_buffer.py:6-254): a scheme-driven dict of
[batch, time, (agents), *vshape] tensors with a `filled` mask, slicing, the one-hot preprocess hook, and a ring replay
buffer with uniform sampling.  Written for device-resident rollouts: `update` accepts tensors already on the device and
copies them without a host round trip; list / numpy inputs are converted exactly like the reference does."""
from types import SimpleNamespace

import numpy as np
import torch as th

from .. import ops


def _count(idx, size):
    if isinstance(idx, slice):
        return len(range(*idx.indices(size)))
    return len(idx)


class EpisodeBatch:
    # the sampler extras' defaults live on the class as well: `del batch.priority` takes an extra off a batch and it reads None again
    reward_norm = priority = priority_log = None

    def __init__(self, scheme, groups, batch_size, max_seq_length, data=None, preprocess=None, device="cpu"):
        self.scheme = dict(scheme)
        self.groups = groups
        self.batch_size = batch_size
        self.max_seq_length = max_seq_length
        self.preprocess = {} if preprocess is None else preprocess
        self.device = device
        # what a sampler tells the learner about the sample (None: nothing): the length the rewards are divided by (gather_windows), the
        # (table, ids, weights) of a prioritised draw and its four logged values (sample_prioritized).  A slice carries none of them.
        self.reward_norm = self.priority = self.priority_log = None
        if data is not None:
            self.data = data
        else:
            self.data = SimpleNamespace(transition_data={}, episode_data={})
            self._allocate(self.scheme, groups, batch_size, max_seq_length, self.preprocess)

    # ---- allocation ------------------------------------------------------------------------------------------
    def _allocate(self, scheme, groups, batch_size, max_seq_length, preprocess):
        for key, (new_key, transforms) in (preprocess or {}).items():
            assert key in scheme
            vshape, dtype = self.scheme[key]["vshape"], self.scheme[key].get("dtype", th.float32)
            for tr in transforms:
                vshape, dtype = tr.infer_output_info(vshape, dtype)
            entry = {"vshape": vshape, "dtype": dtype}
            for opt in ("group", "episode_const"):
                if opt in self.scheme[key]:
                    entry[opt] = self.scheme[key][opt]
            self.scheme[new_key] = entry
        assert "filled" not in scheme, '"filled" is a reserved key for masking.'
        scheme.update({"filled": {"vshape": (1,), "dtype": th.long}})
        for key, info in scheme.items():
            assert "vshape" in info, "Scheme must define vshape for {}".format(key)
            vshape = info["vshape"]
            vshape = (vshape,) if isinstance(vshape, int) else tuple(vshape)
            group = info.get("group", None)
            if group:
                assert group in groups, "Group {} must have its number of members defined in _groups_".format(group)
                vshape = (groups[group],) + vshape
            dtype = info.get("dtype", th.float32)
            if info.get("episode_const", False):
                self.data.episode_data[key] = th.zeros((batch_size,) + vshape, dtype=dtype, device=self.device)
            else:
                self.data.transition_data[key] = th.zeros((batch_size, max_seq_length) + vshape, dtype=dtype, device=self.device)

    def extend(self, scheme, groups=None):
        self._allocate(scheme, self.groups if groups is None else groups, self.batch_size, self.max_seq_length, None)

    def take_extras(self, other):
        """carry other's sampler extras (a learner's static batch stands for the batch it was captured on)"""
        self.reward_norm, self.priority, self.priority_log = other.reward_norm, other.priority, other.priority_log
        return self

    def to(self, device):
        for store in (self.data.transition_data, self.data.episode_data):
            for k in store:
                store[k] = store[k].to(device)
        self.device = device

    # ---- writes ----------------------------------------------------------------------------------------------
    def update(self, data, bs=slice(None), ts=slice(None), mark_filled=True):
        slices = self._parse_slices((bs, ts))
        for k, v in data.items():
            if k in self.data.transition_data:
                target, sl = self.data.transition_data, tuple(slices)
                if mark_filled:
                    target["filled"][sl] = 1
                    mark_filled = False
            elif k in self.data.episode_data:
                target, sl = self.data.episode_data, slices[0]
            else:
                raise KeyError("{} not found in transition or episode data".format(k))
            dtype = self.scheme[k].get("dtype", th.float32)
            if isinstance(v, th.Tensor):
                v = v.detach().to(device=self.device, dtype=dtype)
            else:
                v = th.tensor(np.asarray(v), dtype=dtype, device=self.device)
            dest = target[k][sl]
            self._check_safe_view(v, dest)
            target[k][sl] = v.reshape(dest.shape)
            if k in self.preprocess:
                new_k, transforms = self.preprocess[k]
                out = target[k][sl]
                for tr in transforms:
                    out = tr.transform(out)
                target[new_k][sl] = out.reshape(target[new_k][sl].shape)

    @staticmethod
    def _check_safe_view(v, dest):
        idx = v.dim() - 1
        for s in dest.shape[::-1]:
            if idx < 0 or v.shape[idx] != s:
                if s != 1:
                    raise ValueError("Unsafe reshape of {} to {}".format(tuple(v.shape), tuple(dest.shape)))
            else:
                idx -= 1

    # ---- reads -----------------------------------------------------------------------------------------------
    def __getitem__(self, item):
        if isinstance(item, str):
            if item in self.data.episode_data:
                return self.data.episode_data[item]
            if item in self.data.transition_data:
                return self.data.transition_data[item]
            raise ValueError(item)
        if isinstance(item, tuple) and all(isinstance(it, str) for it in item):
            nd = SimpleNamespace(transition_data={}, episode_data={})
            for key in item:
                if key in self.data.transition_data:
                    nd.transition_data[key] = self.data.transition_data[key]
                elif key in self.data.episode_data:
                    nd.episode_data[key] = self.data.episode_data[key]
                else:
                    raise KeyError("Unrecognised key {}".format(key))
            scheme = {key: self.scheme[key] for key in item}
            groups = {self.scheme[key]["group"]: self.groups[self.scheme[key]["group"]] for key in item if "group" in self.scheme[key]}
            return EpisodeBatch(scheme, groups, self.batch_size, self.max_seq_length, data=nd, device=self.device)
        sl = self._parse_slices(item)
        nd = SimpleNamespace(transition_data={}, episode_data={})
        for k, v in self.data.transition_data.items():
            nd.transition_data[k] = v[tuple(sl)]
        for k, v in self.data.episode_data.items():
            nd.episode_data[k] = v[sl[0]]
        return EpisodeBatch(self.scheme, self.groups, _count(sl[0], self.batch_size), _count(sl[1], self.max_seq_length),
                            data=nd, device=self.device)

    def _parse_slices(self, items):
        if isinstance(items, (slice, int, list, np.ndarray, th.Tensor)):
            items = (items, slice(None))
        if isinstance(items[1], list):
            raise IndexError("Indexing across Time must be contiguous")
        parsed = []
        for it in items:
            if isinstance(it, (list, np.ndarray)):      # one host -> device transfer of the indices, not one per field
                it = th.as_tensor(np.asarray(it), dtype=th.long, device=self.device)
            parsed.append(slice(it, it + 1) if isinstance(it, int) else it)
        return parsed

    def max_t_filled(self):
        return th.sum(self.data.transition_data["filled"], 1).max(0)[0]

    def __repr__(self):
        return "EpisodeBatch. Batch Size:{} Max_seq_len:{} Keys:{} Groups:{}".format(
            self.batch_size, self.max_seq_length, self.scheme.keys(), self.groups.keys())


class ReplayBuffer(EpisodeBatch):
    def __init__(self, scheme, groups, buffer_size, max_seq_length, preprocess=None, device="cpu"):
        super().__init__(scheme, groups, buffer_size, max_seq_length, preprocess=preprocess, device=device)
        self.buffer_size = buffer_size
        self.buffer_index = 0
        self.episodes_in_buffer = 0
        # device-resident buffers draw their sample indices on the device (ops.sample_ids: counter generator keyed by a seed taken
        # from numpy's global generator at the first device sample -- np.random.seed still makes a run reproducible -- and the
        # number of the sample call); host buffers keep the reference's np.random.choice and consume nothing else
        self._sample_seed = None
        self._sample_calls = 0
        # the draws' persistent tensors (_draw_tensors): ids / t0 int64 [batch_size]; weights f32 [batch_size] and log f32 [4] exist only
        # once a prioritised draw was made
        self._draws = SimpleNamespace(ids=None, t0=None, entries=None, weights=None, log=None)
        # time windows (sample_windows): "episode" | "window", the length a window batch's rewards are divided by (gather_windows)
        self.window_norm = "episode"
        self.last_window_ids = self.last_window_t0 = None
        # prioritised replay (enable_priorities): the fixed-point priority table, one entry per slot; None = the feature is off
        self.priority_table = None
        # a priority per training window (enable_priorities(segments=S, ...)): S entries per slot, entry (slot, k) at slot S + k, and
        # the grid (S, s, last_start) of ops.window_grid the draws map entries with; None = one entry per slot
        self.priority_segments = 1
        self.priority_grid = self.priority_window = None

    def reserve(self, n):
        """A view over the next n episode slots, for producers that write whole episodes in place (vectorised runners): hand
        the filled view to insert_episode_batch, which then only advances the ring indices instead of copying.  None if the
        slots would wrap around."""
        if self.buffer_index + n > self.buffer_size:
            return None
        view = self[self.buffer_index:self.buffer_index + n]
        view._reserved = (self, self.buffer_index)
        return view

    def insert_episode_batch(self, ep_batch, priorities=None):
        """priorities (prioritised replay, per_initial_priority "rollout"): a device int32 tensor of ep_batch.batch_size fixed-point
        priorities the episodes enter the table with -- [n], or [n, S] with a priority per window (one ops.copy_blocks launch per
        contiguous run of slots; split with the batch on wrap-around).  None: the slots' entries are zeroed -- drawn at the table's
        maximum until trained on."""
        n = ep_batch.batch_size
        res = getattr(ep_batch, "_reserved", None)
        if priorities is not None:
            if self.priority_table is None:
                raise ValueError("insert_episode_batch: priorities given, but enable_priorities() was not called")
            want = (n,) if self.priority_grid is None else (n, self.priority_segments)
            if priorities.dtype != th.int32 or tuple(priorities.shape) != want or priorities.device != self.priority_table.device:
                raise ValueError("insert_episode_batch: priorities %s %s on %s: int32 %s on %s expected"
                                 % (tuple(priorities.shape), priorities.dtype, priorities.device, list(want), self.priority_table.device))
        if self.buffer_index + n > self.buffer_size:
            left = self.buffer_size - self.buffer_index
            self.insert_episode_batch(ep_batch[0:left, :], None if priorities is None else priorities[:left])
            self.insert_episode_batch(ep_batch[left:, :], None if priorities is None else priorities[left:])
            return
        if not (res is not None and res[0] is self and res[1] == self.buffer_index):      # (else: written in place, reserve)
            where = slice(self.buffer_index, self.buffer_index + n)
            self.update(ep_batch.data.transition_data, where, slice(0, ep_batch.max_seq_length), mark_filled=False)
            self.update(ep_batch.data.episode_data, where)
        if priorities is None:
            self._reset_priorities(self.buffer_index, n)
        else:
            self._write_priorities(self.buffer_index, priorities)
        self.buffer_index += n
        self.episodes_in_buffer = max(self.episodes_in_buffer, self.buffer_index)
        self.buffer_index %= self.buffer_size

    def can_sample(self, batch_size):
        return self.episodes_in_buffer >= batch_size

    def sample(self, batch_size, out=None):
        """batch_size episodes drawn without replacement (episode_buffer.py:240-244).  out: an EpisodeBatch of batch_size whole
        episodes (a learner's static copy of the sampled batch) that receives the episodes directly -- one gather per field
        instead of a gather into fresh tensors and a second copy into the consumer's buffers; taken only when it lives on the
        buffer's device.  A device-resident buffer draws the indices on the device (ssd_sample_ids): no host draw, no H2D copy."""
        assert self.can_sample(batch_size)
        if self.episodes_in_buffer == batch_size:
            return self[:batch_size]
        if self._draws_on_device(batch_size):
            d = self._draw_tensors(batch_size)
            ids = ops.sample_ids(self._sample_seed, self._sample_calls, self.episodes_in_buffer, batch_size, d.ids)
            self._sample_calls += 1
        else:
            ep_ids = np.random.choice(self.episodes_in_buffer, batch_size, replace=False)   # episode_buffer.py:243
            ids = th.as_tensor(ep_ids, dtype=th.long, device=self.device)
        return self._gather_episodes(ids, out)

    def _draws_on_device(self, batch_size):
        """a device-resident buffer draws batch_size <= SAMPLE_IDS_MAX samples with the draw kernel (else: numpy's generator)"""
        return th.device(self.device).type == "cuda" and batch_size <= ops.abi.SAMPLE_IDS_MAX

    def _draw_tensors(self, batch_size, prioritized=False):
        """The persistent tensors a draw of batch_size samples writes, and the seed the draw is keyed by: taken from numpy's generator by
        the first draw that asks.  The tensors are replaced only when batch_size changes -- a captured train step bakes their addresses
        in -- and weights / log exist only once a prioritised draw asked for them."""
        if self._sample_seed is None:
            self._sample_seed = int(np.random.randint(0, 2 ** 31 - 1)) | (int(np.random.randint(0, 2 ** 31 - 1)) << 32)
        d = self._draws
        if d.ids is None or d.ids.numel() != batch_size:
            idx = th.empty(2, batch_size, dtype=th.long, device=self.device)
            d = self._draws = SimpleNamespace(ids=idx[0], t0=idx[1], entries=None, weights=None, log=None)
        if prioritized and d.weights is None:
            d.weights, d.log = th.empty(batch_size, dtype=th.float32, device=self.device), th.empty(4, dtype=th.float32, device=self.device)
        if prioritized and self.priority_grid is not None and d.entries is None:      # (a priority per window: the drawn table entries)
            d.entries = th.empty(batch_size, dtype=th.long, device=self.device)
        return d

    def _fits(self, out, batch_size, slots):
        """out can receive batch_size samples of `slots` slots each: that shape, every field on the buffer's device, no episode data"""
        return (out is not None and out.batch_size == batch_size and out.max_seq_length == slots and not self.data.episode_data
                and all(out.data.transition_data[k].device == v.device for k, v in self.data.transition_data.items()))

    def _gather_episodes(self, ids, out):
        """the whole episodes ids: gathered into `out` where it fits (device buffers: one launch for all fields), else a fresh batch"""
        if not self._fits(out, ids.numel(), self.max_seq_length):
            return self[ids]
        pairs = [(v, out.data.transition_data[k]) for k, v in self.data.transition_data.items()]
        if not (ids.is_cuda and ops.gather_rows(pairs, ids)):
            ops._leaving_kernels("gather_rows", ids, "fields that do not qualify for ssd_gather_rows")
            for v, dst in pairs:
                th.index_select(v, 0, ids, out=dst)
        return out

    # ---- time windows (config keys train_window / train_burn_in / train_window_norm) -------------------------------------------
    def gather_windows(self, ids, t0, window, burn_in, out=None):
        """An EpisodeBatch of window + 1 slots: row e holds slots [t0[e], t0[e] + window] of episode ids[e] (slot t0 + window is the
        bootstrap slot, as slot T of a whole episode).  The first K_e rows carry no loss, K_e = burn_in if t0[e] > 0 and 0 if
        t0[e] == 0 (there the zero hidden state is the true state), expressed through `filled` alone: filled[e, r] = the stored value
        * (r >= K_e).  The batch carries `reward_norm`, the length the learner divides the rewards by: the episode's slot count
        (window_norm "episode": targets keep their scale whatever the window) or window + 1 ("window": the reference run on the
        slice).  Device buffers: every field in ONE launch (ssd_gather_windows), ids / t0 stay on the device; out: an EpisodeBatch
        of that shape on the buffer's device that receives the windows (a learner's static batch).  The caller guarantees ids within
        the stored episodes and t0 + window < max_seq_length on device tensors; host indices are checked."""
        T = self.max_seq_length - 1
        if not 1 <= window <= T or not 0 <= burn_in < window:
            raise ValueError("gather_windows: window %r outside 1 .. %d or burn_in %r outside 0 .. window - 1" % (window, T, burn_in))
        W = window + 1
        as_idx = lambda x: x.to(device=self.device, dtype=th.long) if isinstance(x, th.Tensor) else th.as_tensor(np.asarray(x), dtype=th.long, device=self.device)
        ids, t0 = as_idx(ids), as_idx(t0)
        B = ids.numel()
        src = self.data.transition_data
        if out is not None and not self._fits(out, B, W):
            raise ValueError("gather_windows: out is not a batch of %d windows of %d slots on the buffer's device" % (B, W))
        if out is None:
            nd = SimpleNamespace(transition_data={k: th.empty((B, W) + tuple(v.shape[2:]), dtype=v.dtype, device=v.device) for k, v in src.items()},
                                 episode_data={k: v[ids] for k, v in self.data.episode_data.items()})
            out = EpisodeBatch(self.scheme, self.groups, B, W, data=nd, device=self.device)
        out.reward_norm = ops.window_reward_norm(self.window_norm, self.max_seq_length, window)
        keys = list(src)
        pairs = [(src[k], out.data.transition_data[k]) for k in keys]
        if ids.is_cuda and ops.gather_windows(pairs, ids, t0, self.max_seq_length, W, burn_in, keys.index("filled")):
            return out
        ops._leaving_kernels("gather_windows", ids, "fields that do not qualify for ssd_gather_windows")
        if not ids.is_cuda and B and not (0 <= int(ids.min()) and int(ids.max()) < self.buffer_size and 0 <= int(t0.min()) and int(t0.max()) + W <= self.max_seq_length):
            raise IndexError("gather_windows: ids or t0 outside the buffer")
        rows = th.arange(W, device=ids.device)
        slots = t0.unsqueeze(1) + rows
        for k, (v, dst) in zip(keys, pairs):
            dst.copy_(v[ids.unsqueeze(1), slots])
        keep = rows.unsqueeze(0) >= th.where(t0 > 0, burn_in, 0).unsqueeze(1)
        out.data.transition_data["filled"].mul_(keep.reshape((B, W) + (1,) * (src["filled"].dim() - 2)).to(src["filled"].dtype))
        return out

    def sample_windows(self, batch_size, window, burn_in, out=None):
        """batch_size windows of `window` transitions, one per sampled episode: the episodes sample() would draw (device buffers:
        the ids of ssd_sample_ids for the same seed and call) and a start t0 uniform on 0 .. T - window each, gathered by
        gather_windows.  Device buffers draw both in ONE launch (ssd_sample_windows); host buffers use numpy's generator.  The drawn
        (ids, t0) stay in last_window_ids / last_window_t0.  With exactly batch_size episodes stored the ids are 0 .. batch_size - 1,
        as in sample(); the starts are still drawn."""
        assert self.can_sample(batch_size)
        n_starts = self.max_seq_length - window
        if n_starts < 1:
            raise ValueError("sample_windows: window %r outside 1 .. %d" % (window, self.max_seq_length - 1))
        if self._draws_on_device(batch_size):
            d = self._draw_tensors(batch_size)
            ids, t0 = ops.sample_windows(self._sample_seed, self._sample_calls, self.episodes_in_buffer, batch_size, n_starts, d.ids, d.t0)
            if self.episodes_in_buffer == batch_size:
                ids.copy_(th.arange(batch_size, device=self.device))
        else:
            ep_ids = np.arange(batch_size) if self.episodes_in_buffer == batch_size else np.random.choice(self.episodes_in_buffer, batch_size, replace=False)
            ids = th.as_tensor(ep_ids, dtype=th.long, device=self.device)
            t0 = th.as_tensor(np.random.randint(0, n_starts, batch_size), dtype=th.long, device=self.device)
        self._sample_calls += 1
        self.last_window_ids, self.last_window_t0 = ids, t0
        return self.gather_windows(ids, t0, window, burn_in, out=out)

    # ---- prioritised replay (config keys prioritized_replay / per_*) --------------------------------------------------------------
    def enable_priorities(self, segments=1, stride=None, window=None):
        """Allocate the priority table: one fixed-point entry per slot (int32 storage of the u32 values of include/ssd_hip.h:
        PRIORITY_ONE = 1.0, 0 = never trained on) on the buffer's device.  From then on every insert zeroes the slots it advances over
        and sample_prioritized can draw.
        window = L with stride = s and segments = S: a priority per training window -- S entries per slot, entry (slot, k) at
        slot S + k for the window starting at min(k s, T - L) (ops.window_grid(T, L, s) must give S); sample_prioritized(window=L) then
        draws entries.  The layout is fixed by the first call."""
        grid = None
        if window is not None:
            grid = ops.window_grid(self.max_seq_length - 1, window, stride or 0)
            if grid[0] != segments or segments > ops.abi.PRIORITY_SEGMENTS_MAX:
                raise ValueError("prioritized replay: segments %r is not the %d windows of length %r at stride %r in %d transitions, or over PRIORITY_SEGMENTS_MAX = %d"
                                 % (segments, grid[0], window, grid[1], self.max_seq_length - 1, ops.abi.PRIORITY_SEGMENTS_MAX))
        elif segments != 1:
            raise ValueError("prioritized replay: segments %r without a window" % (segments,))
        if self.buffer_size * segments > ops.abi.PRIORITY_POP_MAX:
            raise ValueError("prioritized replay: buffer_size %d * %d entries over PRIORITY_POP_MAX = %d" % (self.buffer_size, segments, ops.abi.PRIORITY_POP_MAX))
        if self.priority_table is None:
            self.priority_segments, self.priority_grid, self.priority_window = segments, grid, window
            self.priority_table = th.zeros(self.buffer_size * segments, dtype=th.int32, device=self.device)
        elif (self.priority_segments, self.priority_grid) != (segments, grid):
            raise ValueError("prioritized replay: the table exists with %d entries per slot (grid %r)" % (self.priority_segments, self.priority_grid))
        return self.priority_table

    def _reset_priorities(self, start, n):
        """the n slots from `start` hold new episodes: their entries go back to 0 (one ssd_fill_blocks launch on the device)"""
        if self.priority_table is not None and n > 0:
            S = self.priority_segments
            ops.fill_blocks([(self.priority_table[start * S:(start + n) * S], 0)])

    def _write_priorities(self, start, priorities):
        """the slots from `start` hold new episodes that bring their priorities along (one ssd_copy_blocks launch on the device)"""
        S = self.priority_segments
        dst = self.priority_table[start * S:start * S + priorities.numel()]
        priorities = priorities.reshape(-1)
        if dst.is_cuda:
            ops.copy_blocks([(priorities.contiguous(), dst)])
        else:
            dst.copy_(priorities)

    def sample_prioritized(self, batch_size, window=0, burn_in=0, beta=0.4, out=None):
        """batch_size samples drawn in proportion to the priority table (stratified, with replacement: duplicate ids are legal; no
        episodes_in_buffer == batch_size shortcut), whole episodes (window 0) or windows of `window` transitions with a uniform start
        each -- ONE launch on a device buffer (ssd_priority_sample), then the gather of sample() / gather_windows.  The batch comes
        back with batch.priority = (table, ids, weights): the table, the drawn ids (int64) and the importance weights (f32,
        (population qeff / total)^(-beta) over their maximum), and batch.priority_log (f32 [4]: mean and max priority, smallest
        weight, distinct ids).  Ids, weights and log live in tensors that persist across calls: a captured train step sees stable
        addresses.  The learner writes the new priorities back in its train step (ops.priority_update).
        With a priority per window (enable_priorities(segments=S, ...)) the draw is over table entries: a drawn entry f is window
        f % S of episode f // S -- no start is drawn, several strata in one episode are several windows of it -- and
        batch.priority = (table, entries, weights): the learner's update writes table[entries[e]] without knowing the layout."""
        assert self.can_sample(batch_size)
        if self.priority_table is None:
            raise ValueError("sample_prioritized: enable_priorities() was not called")
        if batch_size > ops.abi.SAMPLE_IDS_MAX:
            raise ValueError("sample_prioritized: batch_size %d over SAMPLE_IDS_MAX = %d" % (batch_size, ops.abi.SAMPLE_IDS_MAX))
        n_starts = self.max_seq_length - window if window else 1
        if n_starts < 1 or window < 0:
            raise ValueError("sample_prioritized: window %r outside 0 .. %d" % (window, self.max_seq_length - 1))
        if self.priority_grid is not None and window != self.priority_window:
            raise ValueError("sample_prioritized: the table holds priorities of windows of %r transitions, window %r asked" % (self.priority_window, window))
        d = self._draw_tensors(batch_size, prioritized=True)
        ops.priority_sample(self._sample_seed, self._sample_calls, self.priority_table, self.episodes_in_buffer * self.priority_segments, batch_size,
                            n_starts, beta, d.ids, d.t0, d.weights, d.log, segments=self.priority_grid, entries_out=d.entries)
        self._sample_calls += 1
        if window:
            self.last_window_ids, self.last_window_t0 = d.ids, d.t0
            batch = self.gather_windows(d.ids, d.t0, window, burn_in, out=out)
        else:
            batch = self._gather_episodes(d.ids, out)
        batch.priority, batch.priority_log = (self.priority_table, d.ids if self.priority_grid is None else d.entries, d.weights), d.log
        return batch

    def sample_latest(self, batch_size):
        ep_ids = np.arange(self.buffer_index - batch_size, self.buffer_index) % self.buffer_size
        return self[ep_ids]

    def __repr__(self):
        return "ReplayBuffer. {}/{} episodes. Keys:{} Groups:{}".format(
            self.episodes_in_buffer, self.buffer_size, self.scheme.keys(), self.groups.keys())
