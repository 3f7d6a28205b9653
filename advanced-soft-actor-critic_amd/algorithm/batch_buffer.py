"""HBM-resident episode batch queue: the drop-in for the reference's `BatchBuffer` (reference
`algorithm/batch_buffer.py`, `utils/operators.py:105-206` `episode_to_batch`), the training mode of
`SAC_Base(use_replay_buffer=False)`.

The reference expands every episode on the host into all of its overlapping `burn_in + n_step (+ 1)` windows,
shuffles them, queues whole NumPy batches and copies one to the device per train step.  Here:

  * window pool   one tensor per key [P, L, *shape] in HBM, L = burn_in + n_step + 1, P = (max_size + 1) * batch_size;
                  every live window is stored once, already padded, in the dtype the replay ring would keep
                  (uint8 images stay uint8 and are widened when a batch is gathered)
  * queue         i32[max_size + 1, batch_size] pool slots of the queued batches (a ring) + i32[1] device head: the
                  absolute number of the next batch to pop
  * BatchPlanner  the host side: forms the window list of every `put_episode` (the carried-over rest first), draws the
                  permutation, cuts batches, applies the drop-oldest rule and gives pool slots only to the new windows
                  that survive.  It never reads from the device: its mirror of the queue answers "is there a batch?"

`put_episode` is ONE launch (`asac_batch_put`: the episode -> its surviving windows' pool slots, the new queue rows, the
head); a batch is ONE launch (`asac_batch_pop_gather`: queue[head] -> dense [B, L] tensors), captured inside the train
step.  At most `max_size` queued batches plus a rest of fewer than `batch_size` windows are live at any moment, so P
slots always suffice and the pool never grows.
"""
from collections import deque

import numpy as np
import torch

from asac_amd import native

__all__ = ['BatchPlanner', 'BatchBuffer']


class BatchPlanner:
    """Host bookkeeping of the batch queue (pure Python: testable without a device).

    Slots are ints in [0, P).  Batch numbers are absolute: the n-th batch ever formed has number n and queue row
    n % (max_size + 1); `head` is the number of the next batch to pop, so the queued batches are [head, tail)."""

    def __init__(self, batch_size: int, max_size: int = 10, permutation=None):
        self.batch_size = int(batch_size)
        self.max_size = int(max_size)
        self.ring_rows = self.max_size + 1
        self.pool_slots = self.ring_rows * self.batch_size
        self.permutation = permutation if permutation is not None else np.random.permutation
        self._free = list(range(self.pool_slots - 1, -1, -1))     # (pop() hands out the lowest first)
        self.rest: list[int] = []                                 # pool slots of the carried-over windows
        self.queue: deque = deque()                               # slot lists of the queued batches, oldest first
        self.head = 0
        self.tail = 0
        self.tags = [None] * self.pool_slots                      # caller's identity of the window in each slot

    def __len__(self) -> int:
        return len(self.queue)

    def _free_slots(self, slots) -> None:
        for s in slots:
            self.tags[s] = None
        self._free.extend(slots)

    def live_slots(self) -> list[int]:
        return [s for b in self.queue for s in b] + list(self.rest)

    def put(self, n_new: int, tags=None):
        """Plan one episode of `n_new` new windows.  -> None (nothing to do) or a dict:
        win_start / win_slot  the surviving new windows (their index among the new ones, their pool slot)
        queue_rows / queue_slots  the queue rows to write and their slots;  head  the head after the put"""
        if n_new <= 0:
            return None
        B = self.batch_size
        items = [(-1, s) for s in self.rest] + [(i, -1) for i in range(n_new)]     # (new index, slot of an old one)
        N = len(items)
        idx = self.permutation(N)
        items = [items[int(k)] for k in idx]
        n_full = N // B
        batches = [items[i * B:(i + 1) * B] for i in range(n_full)]
        rest = items[n_full * B:]
        # drop-oldest: the queue keeps the last `max_size` of (queued + new) batches
        n_drop = max(0, len(self.queue) + n_full - self.max_size)
        drop_old = min(n_drop, len(self.queue))
        for _ in range(drop_old):
            self._free_slots(self.queue.popleft())
            self.head += 1
        drop_new = n_drop - drop_old
        for b in batches[:drop_new]:          # formed and dropped at once: only their carried-over windows held slots
            self._free_slots([s for i, s in b if i < 0])
            self.tail += 1
            self.head += 1
        win_start, win_slot = [], []

        def place(group):
            slots = []
            for i, s in group:
                if i >= 0:
                    s = self._free.pop()
                    win_start.append(i)
                    win_slot.append(s)
                    if tags is not None:
                        self.tags[s] = tags[i]
                slots.append(s)
            return slots

        queue_rows, queue_slots = [], []
        for b in batches[drop_new:]:
            slots = place(b)
            self.queue.append(slots)
            queue_rows.append(self.tail % self.ring_rows)
            queue_slots.append(slots)
            self.tail += 1
        self.rest = place(rest)
        assert len(self.queue) == self.tail - self.head <= self.max_size
        return dict(win_start=win_start, win_slot=win_slot, queue_rows=queue_rows, queue_slots=queue_slots,
                    head=self.head)

    def pop(self):
        """-> the slots of the oldest queued batch (freed at once: the device reads them in stream order, before any
        later put can write them), or None"""
        if not self.queue:
            return None
        slots = self.queue.popleft()
        self.head += 1
        self._free_slots(slots)
        return slots


def _f32_bits(x: float) -> int:
    return int(np.float32(x).view(np.uint32))


def _pad_of(dtype: torch.dtype, value: float):
    """(pad_mode, pad_word) filling every element of a `dtype` row with `value` (0 or 1)"""
    if dtype == torch.bool or (dtype in (torch.uint8, torch.int8)):
        return native.PAD_BYTE, int(value)
    if value == 0:
        return native.PAD_WORD, 0
    if dtype == torch.float32:
        return native.PAD_WORD, _f32_bits(value)
    if dtype == torch.int32:
        return native.PAD_WORD, int(value) & 0xffffffff
    raise TypeError(f'no padding word for {dtype} = {value}')


class BatchBuffer:
    """reference `BatchBuffer` (batch_buffer.py) with the queue in HBM.  `put_episode` / `get_batch` as the reference;
    the episode's arrays may also be device tensors (the device-resident agent's episode slabs)."""

    def __init__(self,
                 burn_in_step: int,
                 n_step: int,
                 padding_action,
                 batch_size: int,
                 device: torch.device | None = None,
                 max_size: int = 10,
                 obs_names: list[str] | None = None,
                 permutation=None):
        self.burn_in_step = int(burn_in_step)
        self.n_step = int(n_step)
        self.batch_size = int(batch_size)
        self.max_size = int(max_size)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if self.device.type != 'cuda':
            raise native.AsacNativeError(f'BatchBuffer is HBM-resident: it needs a cuda (ROCm) device, got {self.device}')
        native.load()
        self.obs_names = None if obs_names is None else list(obs_names)
        self.L = self.burn_in_step + self.n_step + 1
        self.planner = BatchPlanner(batch_size, max_size, permutation)
        pad = padding_action if isinstance(padding_action, torch.Tensor) else torch.from_numpy(np.asarray(padding_action))
        self._pad_action = pad.reshape(-1).to(self.device, torch.float32).contiguous()
        with torch.cuda.device(self.device):
            self._queue = torch.zeros((self.planner.ring_rows, self.batch_size), dtype=torch.int32, device=self.device)
            self._head = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._pool: dict[str, torch.Tensor] | None = None
        self._batch: dict[str, torch.Tensor] | None = None      # the step's static batch [B, L, *] (f32 observations)
        self._static_keys = None
        self._staging = None

    @property
    def permutation(self):
        return self.planner.permutation

    @permutation.setter
    def permutation(self, fn):
        self.planner.permutation = fn

    def __len__(self) -> int:
        return len(self.planner)

    @property
    def has_batch(self) -> bool:
        return len(self.planner) > 0

    def _obs_key(self, j: int) -> str:
        return f'obs_{self.obs_names[j]}' if self.obs_names is not None else f'obs_{j}'

    # ------------------------------------------------------------------------------------------
    # ingress
    # ------------------------------------------------------------------------------------------
    def _rows(self, ep_indexes, ep_last_masks, ep_obses_list, ep_actions, ep_rewards, ep_dones, ep_probs,
              ep_pre_seq_hidden_states) -> dict:
        rows = {'index': ep_indexes[0], 'last_mask': ep_last_masks[0]}
        for j, o in enumerate(ep_obses_list):
            rows[self._obs_key(j)] = o[0]
        rows.update(action=ep_actions[0], reward=ep_rewards[0], done=ep_dones[0], mu_prob=ep_probs[0],
                    pre_seq_hidden_state=ep_pre_seq_hidden_states[0])
        return rows

    def _build_pool(self, rows: dict) -> None:
        P, L = self.planner.pool_slots, self.L
        pool = {}
        with torch.cuda.device(self.device):
            for k, v in rows.items():
                dtype = v.dtype if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v)[:0]).dtype
                pool[k] = torch.zeros((P, L, *v.shape[1:]), dtype=dtype, device=self.device)
                if k == 'last_mask':
                    pool['padding_mask'] = torch.zeros((P, L), dtype=torch.bool, device=self.device)
        assert pool['index'].dtype == torch.int32, 'index rows are int32'
        assert pool['action'].dtype == torch.float32 and pool['action'].shape[2:] == self._pad_action.shape, \
            'actions are f32 rows of the padding action\'s width'
        assert len(pool) <= native.MAX_GATHER_KEYS, 'too many transition keys for one launch'
        self._pool = pool
        self._specs = []
        for k, col in pool.items():
            row_bytes = col.element_size() * int(np.prod(col.shape[2:], dtype=np.int64))
            if k == 'padding_mask':
                self._specs.append(dict(key=k, pool=col, row_bytes=1, pad_mode=native.PAD_EMIT_MASK))
                continue
            if row_bytes == 0:
                continue      # (no hidden state: nothing to move)
            pad_row = None
            if k == 'index':
                mode, word = native.PAD_WORD, 0xffffffff
            elif k == 'action':
                mode, word, pad_row = native.PAD_ROW, 0, self._pad_action
            elif k in ('last_mask', 'done'):
                mode, word = _pad_of(col.dtype, 1)
            elif k == 'mu_prob':
                mode, word = _pad_of(col.dtype, 1.)
            else:        # observations, reward, hidden state
                mode, word = native.PAD_WORD, 0
            self._specs.append(dict(key=k, pool=col, row_bytes=row_bytes, pad_mode=mode, pad_word=word, pad_row=pad_row))

    def _stage(self, nbytes: int) -> dict:
        """pinned host buffer + its device twin, grown as needed; the host side is reused only after the previous copy
        out of it has completed"""
        st = self._staging
        if st is None or st['host'].numel() < nbytes:
            size = max(1 << 16, 1 << (int(nbytes) - 1).bit_length())
            host = torch.empty(size, dtype=torch.uint8).pin_memory()
            st = self._staging = {'host': host, 'host_np': host.numpy(), 'event': torch.cuda.Event(),
                                  'dev': torch.empty(size, dtype=torch.uint8, device=self.device)}
        else:
            st['event'].synchronize()
        return st

    def put_episode(self,
                    ep_indexes,
                    ep_last_masks,
                    ep_obses_list,
                    ep_actions,
                    ep_rewards,
                    ep_dones,
                    ep_probs,
                    ep_pre_seq_hidden_states,
                    tags=None) -> None:
        """reference BatchBuffer.put_episode: every array [1, ep_len, *] (NumPy, or device tensors).  `tags`: optional
        per-window identities kept by the planner (tests)."""
        rows = self._rows(ep_indexes, ep_last_masks, ep_obses_list, ep_actions, ep_rewards, ep_dones, ep_probs,
                          ep_pre_seq_hidden_states)
        T = int(rows['index'].shape[0])
        if self._pool is None:
            self._build_pool(rows)
        plan = self.planner.put(T - 1, tags)
        if plan is None:
            return
        n_win, n_q, B = len(plan['win_slot']), len(plan['queue_rows']), self.batch_size
        ints = np.concatenate([np.asarray(plan['win_start'], np.int64) - self.burn_in_step,
                               np.asarray(plan['win_slot'], np.int64),
                               np.asarray(plan['queue_rows'], np.int64),
                               np.asarray(plan['queue_slots'], np.int64).reshape(-1)]).astype(np.int32)
        on_device = isinstance(rows['index'], torch.Tensor)
        offs, total = {}, 0
        if not on_device:
            arrs = {}
            for s in self._specs:
                k = s['key']
                if k == 'padding_mask':
                    continue
                col = self._pool[k]
                v = np.ascontiguousarray(rows[k])
                want = torch.empty(0, dtype=col.dtype).numpy().dtype
                if v.dtype != want:
                    v = np.ascontiguousarray(v.astype(want))
                if tuple(v.shape) != (T, *col.shape[2:]):
                    raise ValueError(f'episode key {k!r}: shape {tuple(v.shape)}, expected {(T, *col.shape[2:])}')
                arrs[k] = v
                offs[k] = total
                total += (v.nbytes + 15) & ~15
        int_off = total
        total += ints.nbytes
        with torch.cuda.device(self.device):
            st = self._stage(total)
            host = st['host_np']
            if not on_device:
                for k, v in arrs.items():
                    host[offs[k]:offs[k] + v.nbytes] = v.reshape(-1).view(np.uint8)
            host[int_off:int_off + ints.nbytes] = ints.view(np.uint8)
            dev = st['dev']
            dev[:total].copy_(st['host'][:total], non_blocking=True)
            st['event'].record()
            plan_dev = dev[int_off:int_off + ints.nbytes].view(torch.int32)
            specs = []
            for s in self._specs:
                k = s['key']
                spec = dict(s)
                if k == 'padding_mask':
                    spec['src'] = None
                elif on_device:
                    col = self._pool[k]
                    # (a temporary is safe: the caching allocator hands its memory out again only to later work on
                    # this stream)
                    v = rows[k].to(self.device, col.dtype).reshape(T, *col.shape[2:]).contiguous()
                    spec['src'], spec['src_stride'] = v, s['row_bytes']
                else:
                    spec['src'], spec['src_stride'] = dev[offs[k]:], s['row_bytes']
                specs.append(spec)
            native.batch_put(native.make_batch_put_keys(specs), T, self.burn_in_step, self.L,
                             plan_dev[:n_win], plan_dev[n_win:2 * n_win], n_win, self.planner.pool_slots,
                             plan_dev[2 * n_win:2 * n_win + n_q], plan_dev[2 * n_win + n_q:], n_q, B,
                             self._queue, self._head, plan['head'])

    # ------------------------------------------------------------------------------------------
    # egress
    # ------------------------------------------------------------------------------------------
    def _gather_specs(self, out: dict, convert: bool):
        specs = []
        for k, col in self._pool.items():
            row_bytes = col.element_size() * int(np.prod(col.shape[2:], dtype=np.int64))
            if row_bytes == 0:
                continue
            cvt = native.CVT_NONE
            if convert and k.startswith('obs_') and col.dtype in (torch.uint8, torch.bool):
                cvt = native.CVT_U8_TO_F32_UNIT if col.dtype == torch.uint8 else native.CVT_BOOL_TO_F32
            specs.append(dict(pool=col, dst=out[k], row_bytes=row_bytes, convert=cvt))
        return specs

    def _alloc(self, convert: bool) -> dict:
        out = {}
        for k, col in self._pool.items():
            dtype = col.dtype
            if convert and k.startswith('obs_') and dtype in (torch.uint8, torch.bool):
                dtype = torch.float32
            out[k] = torch.zeros((self.batch_size, self.L, *col.shape[2:]), dtype=dtype, device=self.device)
        return out

    def build_static(self) -> dict:
        """the step's static batch: {key: [B, L, *]} with f32 observations, the keys and layout `SAC_Base._step_sample`
        reads from the replay buffer's batch"""
        if self._batch is None:
            assert self._pool is not None, 'no episode has been put yet'
            with torch.cuda.device(self.device):
                self._batch = self._alloc(convert=True)
            self._static_specs = self._gather_specs(self._batch, convert=True)
            self._static_keys = native.make_batch_gather_keys(self._static_specs)
        return self._batch

    def gather_into_static(self) -> None:
        """device work of a pop (capturable): queue[head] -> the static batch.  The head is advanced by
        `advance_head` after the step's last launch."""
        native.batch_pop_gather(self._static_keys, self._queue, self._head, self.batch_size, self.L,
                                self.planner.pool_slots)

    def advance_head(self) -> None:
        self._head.add_(1)

    def pop_host(self) -> None:
        """host side of a pop the device does inside the step"""
        assert self.planner.pop() is not None

    def get_batch(self):
        """reference BatchBuffer.get_batch: None, or (bn_indexes, bn_last_masks, bn_padding_masks, bnx_obses_list,
        bn_actions, bn_rewards, bn_dones, bn_probs, bnx_pre_seq_hidden_states) as fresh device tensors (observations in
        their stored dtype, as the reference returns them)"""
        if not self.has_batch:
            return None
        with torch.cuda.device(self.device):
            out = self._alloc(convert=False)
            native.batch_pop_gather(native.make_batch_gather_keys(self._gather_specs(out, convert=False)), self._queue,
                                    self._head, self.batch_size, self.L, self.planner.pool_slots)
            self.advance_head()
        self.planner.pop()
        obs_keys = [k for k in out if k.startswith('obs_')]
        bn = lambda k: out[k][:, :-1]  # noqa: E731
        return (bn('index'), bn('last_mask'), bn('padding_mask'), [out[k] for k in obs_keys], bn('action'), bn('reward'),
                bn('done'), bn('mu_prob'), out['pre_seq_hidden_state'])

    def close(self) -> None:
        pass
