"""Per-device buffer pools of the head: the grow-only scratch workspace of every (device, stream) and the pinned range-status
words of the split-fp16 kernels.  Both live for the life of the process; ``Os2dHead.forward`` (head.py) draws from them."""
import os
import weakref

import torch


_WORKSPACES = {}


def workspace_cap_bytes():
    """Upper bound of ONE scratch buffer (classes are processed in chunks that fit).  An MI355X has 288 GB of HBM3E, so
    the default is generous: 16 GiB holds ~1150 classes at 60x80 in one chunk (all 1024 classes of BASELINE.json's
    configs[2] in a single pass of large launches)."""
    return int(float(os.environ.get("OS2D_WORKSPACE_GB", "16")) * (1 << 30))


def workspace_total_cap_bytes():
    """Upper bound of ALL scratch buffers of a device together (one per HIP stream in use: 7 for the pyramid runner)."""
    return int(float(os.environ.get("OS2D_WORKSPACE_TOTAL_GB", "96")) * (1 << 30))


RANGE_WORDS_ZEROED = 1024      # words (4096 bytes) zero-filled at the start of every new workspace, whatever the call


def range_words_bytes(images):
    """Bytes to zero-fill at the start of a NEW workspace for a head call on ``images`` feature maps: its (A + 1) range words
    (include/os2d_hip.h, ``status``), never less than the fixed ``RANGE_WORDS_ZEROED`` words."""
    return 4 * max(int(images) + 1, RANGE_WORDS_ZEROED)


def get_workspace(device, wanted, minimum, images=0):
    """Grow-only scratch buffer, one per (device, stream): concurrent heads on different HIP streams (the pyramid
    runner) must not share intermediates.  The pyramid runner draws its streams from a fixed pool
    (os2d_amd/engine/pyramid.py), so the number of buffers is bounded by the number of level slots; their total is kept
    below ``workspace_total_cap_bytes`` by shrinking what a NEW or growing buffer may take (never below ``minimum``, the
    footprint of one class).  ``images``: A of the head call the buffer is for.  A new buffer is zero-filled over that call's
    A + 1 range words (a fixed 4096 bytes covered A <= 1023 only), and a buffer that is REUSED by a call with
    more words than it was ever filled for gets the missing words zeroed (on the stream of the key, ahead of the call): the
    words of a call have then been zero at least once.  What this does not do: between calls the words inside the filled extent
    may hold an earlier call's epochs or - where a call with fewer images carved its intermediates there - its data; such a
    stale word matches a later call's epoch with probability 2^-32 (the epochs start at a random base, head_call.hip)."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (device.type, index, torch.cuda.current_stream(device).cuda_stream)
    buf = _WORKSPACES.get(key)
    others = sum(b.numel() for k, b in _WORKSPACES.items() if b is not None and k != key and k[1] == index)
    room = max(workspace_total_cap_bytes() - others, 0)
    size = max(min(wanted, workspace_cap_bytes(), room), minimum)
    if buf is None or buf.numel() < size:
        _WORKSPACES[key] = None
        buf = torch.empty(size, dtype=torch.uint8, device=device)
        buf.range_bytes_zeroed = min(range_words_bytes(images), size)
        buf[:buf.range_bytes_zeroed].zero_()       # the range words of a head call live at the start of its workspace (include/os2d_hip.h)
        _WORKSPACES[key] = buf
    else:
        need, have = min(range_words_bytes(images), buf.numel()), getattr(buf, "range_bytes_zeroed", 0)
        if need > have:
            buf[have:need].zero_()
            buf.range_bytes_zeroed = need
    return buf


def release_workspaces():
    _WORKSPACES.clear()


_STATUS_WORDS = {}
STATUS_SLOTS = 1024


class _StatusSlots(object):
    """The range-status words of one device: pinned arrays of ``STATUS_SLOTS`` int32 that are never freed, a free list, and
    one slot per LIVE head."""

    def __init__(self):
        self.arrays = []
        self.free = []

    def take(self):
        if not self.free:
            words = torch.zeros(STATUS_SLOTS, dtype=torch.int32).pin_memory()
            self.arrays.append(words)
            self.free.extend(words[i:i + 1] for i in range(STATUS_SLOTS - 1, -1, -1))
        word = self.free.pop()
        word[0] = 0
        return word

    def give_back(self, word):
        self.free.insert(0, word)          # reused last: kernels of the head that owned it have long drained by then


def device_status_word(device, owner=None):
    """A sticky range-status word of the split-fp16 kernels for ONE head: an int32 in mapped pinned host memory.  The words
    of a device live in arrays that are allocated once and kept for the life of the process: kernels in flight store to a
    word through a raw pointer (only when an activation leaves the fp16 range), so the memory must never go back to the host
    allocator while any kernel of any head may still run - a per-head tensor (round 2) could be garbage-collected with its
    head while that head's kernels were still queued.  Every LIVE head owns one word (round 3 shared ONE word
    between all heads of a device: a flag raised by head A's kernels could be consumed and cleared by head B - ADVICE r3; round 4
    handed slots out round-robin and zeroed a recycled slot under its live owner after 1024 heads - ADVICE r4): a word returns
    to the free list when ``owner`` is garbage-collected, goes to the back of that list, and the arrays grow by another
    ``STATUS_SLOTS`` words when every word is owned."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    slots = _STATUS_WORDS.get(index)
    if slots is None:
        slots = _STATUS_WORDS[index] = _StatusSlots()
    word = slots.take()
    if owner is not None:
        weakref.finalize(owner, slots.give_back, word)
    return word
