"""Host side of batched inference from raw frames: which frames share a batch, how they reach the GPU, and how the
next files are decoded while the GPU works.

``plan_batches`` groups consecutive frames whose letterboxed size matches (a batch has one [B,3,H,W] input).
``FrameBatcher`` packs host BGR frames into one of two pinned staging buffers and uploads each batch with one copy
on a side stream; ``prefetch_frames`` decodes image files on a small thread pool ahead of the consumer.
The device work on the frames is ``yolov6.hip.runtime.detect_frames``.
"""
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from yolov6.data.data_augment import letterbox_geometry
from yolov6.utils.nv12 import Nv12Frame, is_nv12_list

MAX_DECODE_THREADS = 8


def letterbox_placement(shape, img_size, stride, auto=True):
    """(rh, rw, top, left, H, W): where a frame of ``shape`` (h, w[, c]) lands in its network input -- resized to (rh, rw),
    at (top, left) of the (H, W) it letterboxes to (reference letterbox arithmetic)."""
    _, (rw, rh), (top, bottom, left, right), _ = letterbox_geometry(tuple(shape[:2]), img_size, auto=auto, stride=stride)
    return rh, rw, top, left, rh + top + bottom, rw + left + right


def letterbox_hw(shape, img_size, stride, auto=True):
    """(H, W) of the network input that a frame of ``shape`` (h, w[, c]) letterboxes to."""
    return letterbox_placement(shape, img_size, stride, auto)[4:]


def plan_batches(shapes, img_size, stride, batch, auto=True):
    """Group consecutive frames into batches: a group holds at most ``batch`` frames that all letterbox to the same (H, W);
    a change of (H, W) ends a group.  Returns a list of lists of frame indices, in source order.  With ``auto=False``
    every frame letterboxes to exactly ``img_size``, so frames of any sizes share batches."""
    if batch < 1:
        raise ValueError('batch must be >= 1')
    groups, cur, cur_hw = [], [], None
    for i, s in enumerate(shapes):
        hw = letterbox_hw(s, img_size, stride, auto)
        if cur and (hw != cur_hw or len(cur) == batch):
            groups.append(cur)
            cur = []
        cur.append(i)
        cur_hw = hw
    if cur:
        groups.append(cur)
    return groups


class FrameBatcher:
    """Uploads a batch of host frames (uint8 [h,w,3] BGR arrays, or host ``Nv12Frame``s: half the bytes) with one H2D copy and
    returns device views of them (tensors, or device ``Nv12Frame``s whose planes are views: Y, then UV right behind it).

    Two slots alternate; each has a pinned staging buffer and a device buffer.  A batch is packed into its slot's staging
    buffer (after waiting for that buffer's previous copy to finish), copied on the batcher's copy stream once the compute
    stream has consumed what the slot's device buffer held before, and the compute stream (the current stream at ``put``)
    waits on an event recorded behind the copy.  Everything the caller enqueues on the compute stream between one ``put``
    and the next counts as the consumer of that batch's views."""

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.copy_stream = torch.cuda.Stream(self.device)
        self.slots = [dict(host=None, dev=None, copied=None, consumed=None) for _ in range(2)]
        self.k = 0
        self.last = None

    def put(self, frames):
        nv12 = is_nv12_list(frames, 'FrameBatcher.put')
        if nv12:
            if any(f.is_tensor for f in frames):
                raise ValueError('FrameBatcher.put takes host Nv12Frames (numpy planes)')
            sizes = [f.nbytes for f in frames]
        else:
            frames = [np.ascontiguousarray(f) for f in frames]
            for f in frames:
                if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                    raise ValueError('frames must be uint8 [h, w, 3] arrays, got %s %s' % (f.dtype, f.shape))
            sizes = [f.nbytes for f in frames]
        compute = torch.cuda.current_stream(self.device)
        if self.last is not None:          # the work enqueued since the last put is the consumer of that slot's device buffer
            ev = torch.cuda.Event()
            ev.record(compute)
            self.last['consumed'] = ev
        slot = self.slots[self.k]
        self.k ^= 1
        offs, n = [], 0
        for nb in sizes:
            offs.append(n)
            n += (nb + 255) // 256 * 256                # 256-byte aligned frame bases
        if slot['copied'] is not None:
            slot['copied'].synchronize()                # the staging buffer's previous copy has left it
        if slot['host'] is None or slot['host'].numel() < n:
            slot['host'] = torch.empty(max(n, 1), dtype=torch.uint8, pin_memory=True)
        host = slot['host'].numpy()
        for f, o in zip(frames, offs):
            if nv12:                                    # Y rows, then UV rows, packed (a source pitch is dropped here)
                hw = f.h * f.w
                host[o:o + hw].reshape(f.h, f.w)[:] = f.y
                host[o + hw:o + f.nbytes].reshape(f.h // 2, f.w // 2, 2)[:] = f.uv
            else:
                host[o:o + f.nbytes] = f.reshape(-1)
        with torch.cuda.device(self.device):
            if slot['dev'] is None or slot['dev'].numel() < n:
                slot['dev'] = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)   # owned by the compute stream
            dev = slot['dev']
            with torch.cuda.stream(self.copy_stream):
                if slot['consumed'] is not None:
                    self.copy_stream.wait_event(slot['consumed'])
                dev[:n].copy_(slot['host'][:n], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.copy_stream)
            dev.record_stream(self.copy_stream)
            slot['copied'] = ev
            compute.wait_event(ev)
        self.last = slot
        if nv12:
            return [Nv12Frame.from_packed(dev[o:o + f.nbytes], f.h, f.w, f.matrix) for f, o in zip(frames, offs)]
        return [dev[o:o + f.nbytes].view(f.shape) for f, o in zip(frames, offs)]


def prefetch_frames(paths, decode, threads=MAX_DECODE_THREADS, depth=16):
    """Yield ``(decode(path), path)`` in order while up to ``depth`` later paths are decoded on a pool of at most
    ``MAX_DECODE_THREADS`` threads (PIL releases the GIL while it decodes)."""
    threads = max(1, min(int(threads), MAX_DECODE_THREADS))
    it = iter(paths)
    q = deque()
    with ThreadPoolExecutor(threads) as pool:
        def fill():
            while len(q) < max(1, depth):
                p = next(it, None)
                if p is None:
                    return
                q.append((p, pool.submit(decode, p)))
        fill()
        while q:
            p, fut = q.popleft()
            fill()
            yield fut.result(), p
