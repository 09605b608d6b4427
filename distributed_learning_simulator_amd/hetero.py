"""Width-heterogeneous models: how a narrower client model maps onto the global flat row.

HeteroFL (Diao, Ding & Tarokh 2021) lets a weak client train the model at width ratio r: the
first ceil(r * C) channels of every hidden layer.  FedRolex (Alam et al. 2022) rolls that
window across the channels from round to round.  Here every parameter tensor is viewed as a
3-D array [O, I, R] (``SliceView``; a model class declares its views in ``hetero_views()``,
models.py) and a channel dimension that several tensors share is one named *group* with one
shift: local index j of a level stands for global index (shift + j) mod C.  A dimension
without a group (the first layer's inputs, the last layer's outputs) is never scaled.

``HeteroPlan`` turns the views, the levels' width ratios and the groups' shifts into the int32
plan of include/dls_hip.h (``words``, with its device copy from ``device_words``), the
levels' own ``ParameterLayout`` and the per-level slice tables the numpy reference reads.
"""
import collections
import math

import numpy as np
import torch

from .layout import ALIGN, ParameterLayout, _round_up

MAX_LEVELS = 8  # DLS_HETERO_MAX_LEVELS
MAX_K = 1024  # DLS_HETERO_MAX_K
MAX_TENSORS = 4096  # DLS_HETERO_MAX_TENSORS
TILE = 1024  # DLS_HETERO_TILE
MAGIC = 0x48545231  # DLS_HETERO_MAGIC
HEADER_WORDS, TENSOR_WORDS, LEVEL_WORDS = 16, 12, 8
RECORD_WORDS = TENSOR_WORDS + MAX_LEVELS * LEVEL_WORDS

# name and shape of a parameter, its [O, I, R] view, and the channel groups of O and I (None:
# the dimension is never scaled)
SliceView = collections.namedtuple("SliceView", "name shape view out_group in_group")


def vector_view(name, channels, group):
    """A 1-D tensor (bias, batch-norm weight or bias) as [1, C, 1]: a level's part is one run."""
    return SliceView(name, (channels,), (1, channels, 1), None, group)


def level_channels(width, channels):
    """ceil(width * channels) channels, at least 1, in exact arithmetic on the ratio given."""
    return max(1, min(channels, math.ceil(width * channels - 1e-9)))


def check_width(width):
    if isinstance(width, bool) or not isinstance(width, (int, float)) or not 0.0 < width <= 1.0:
        raise ValueError(f"a width ratio must be a number in (0, 1], not {width!r}")
    return float(width)


def _magic(d):
    """(m, s) with floor(n / d) == (n * m >> 32) >> s for every 0 <= n < 2^31; d = 1: (0, 0)."""
    if d == 1:
        return 0, 0
    l = (d - 1).bit_length()
    return (1 << (31 + l)) // d + 1, l - 1


def _compact_shape(shape, Ol, Il, R):
    if len(shape) == 1:
        return (Il,)
    if len(shape) == 2:
        return (Ol, Il * R)
    return (Ol, Il) + tuple(shape[2:])


class HeteroPlan:
    """views: the global model's ``SliceView``s in ``named_parameters`` order; widths: the
    levels' ratios (1 <= len <= MAX_LEVELS, distinct); shifts: {group: shift} (missing: 0)."""

    def __init__(self, views, widths, shifts=None):
        self.views = [SliceView(*v) for v in views]
        self.widths = tuple(check_width(w) for w in widths)
        if not 1 <= len(self.widths) <= MAX_LEVELS:
            raise ValueError(f"fed_hetero takes 1..MAX_LEVELS={MAX_LEVELS} width levels, not "
                             f"{len(self.widths)}")
        if len(set(self.widths)) != len(self.widths):
            raise ValueError(f"the width levels must be distinct, not {self.widths}")
        if not 1 <= len(self.views) <= MAX_TENSORS:
            raise ValueError(f"fed_hetero takes 1..MAX_TENSORS={MAX_TENSORS} tensors, not "
                             f"{len(self.views)}")
        self.groups = {}
        for v in self.views:
            O, I, R = v.view
            if min(O, I, R) < 1 or O * I * R != (math.prod(v.shape) if v.shape else 1):
                raise ValueError(f"{v.name}: the view {v.view} is not the shape {v.shape}")
            for g, C in ((v.out_group, O), (v.in_group, I)):
                if g is not None and self.groups.setdefault(g, C) != C:
                    raise ValueError(f"{v.name}: group {g!r} has {self.groups[g]} channels "
                                     f"elsewhere and {C} here")
        self.layout = ParameterLayout((v.name, v.shape) for v in self.views)
        if self.layout.P >= 1 << 31 or max(self.layout.numels) > 1 << 30:
            raise ValueError("fed_hetero rows are shorter than 2^31 elements, tensors at most 2^30")
        # per level: how many channels of each group, and the level's own layout
        self.level_channels = [{g: level_channels(w, C) for g, C in self.groups.items()}
                               for w in self.widths]
        self.level_layouts = []
        for ch in self.level_channels:
            self.level_layouts.append(ParameterLayout(
                (v.name, _compact_shape(v.shape, ch.get(v.out_group, v.view[0]),
                                        ch.get(v.in_group, v.view[1]), v.view[2]))
                for v in self.views))
        self._device_words = {}
        self.set_shifts(shifts or {})

    @property
    def P(self):
        return self.layout.P

    @property
    def level_P(self):
        return [lay.P for lay in self.level_layouts]

    def level_of(self, width):
        try:
            return self.widths.index(float(width))
        except ValueError:
            raise ValueError(f"width {width!r} is not one of the plan's levels {self.widths}")

    def set_shifts(self, shifts):
        """Rebuild the plan's words for {group: shift}; a shift is taken mod the group's size."""
        unknown = set(shifts) - set(self.groups)
        if unknown:
            raise ValueError(f"shifts for unknown groups {sorted(unknown)}")
        self.shifts = {g: int(shifts.get(g, 0)) % C for g, C in self.groups.items()}
        T, L = len(self.views), len(self.widths)
        words = np.zeros(HEADER_WORDS + T * (1 + RECORD_WORDS), np.int64)
        words[:5] = (MAGIC, T, L, 0, self.layout.P)
        words[8:8 + L] = self.level_P
        self.slices = [[] for _ in range(L)]  # per level and tensor: (loff, Ol, Il, shO, shI)
        tiles = 0
        for t, v in enumerate(self.views):
            O, I, R = v.view
            tiles += -(-_round_up(O * I * R, ALIGN) // TILE)
            words[HEADER_WORDS + t] = tiles
            rec = HEADER_WORDS + T + t * RECORD_WORDS
            fast = (I * R) % 4 == 0
            for l in range(L):
                ch = self.level_channels[l]
                Ol, Il = ch.get(v.out_group, O), ch.get(v.in_group, I)
                # a dimension held whole needs no shift
                shO = self.shifts.get(v.out_group, 0) if Ol < O else 0
                shI = self.shifts.get(v.in_group, 0) if Il < I else 0
                loff = self.level_layouts[l].offsets[t]
                self.slices[l].append((loff, Ol, Il, shO, shI))
                words[rec + TENSOR_WORDS + l * LEVEL_WORDS:][:7] = (loff, Ol, Il, shO, shI, Il * R,
                                                                   Ol * Il * R)
                fast = fast and shO == 0 and shI == 0 and (Il * R) % 4 == 0
            words[rec:rec + TENSOR_WORDS] = (self.layout.offsets[t], O, I, R, *_magic(I * R),
                                             *_magic(R), int(fast), O * I * R, I * R,
                                             _round_up(O * I * R, ALIGN))
        words[3] = tiles
        # the 32-bit constants keep their bits as int32 words
        self.words = torch.from_numpy(words.astype(np.uint32).view(np.int32).copy())
        self._device_words.clear()

    def device_words(self, device):
        """The plan's words on ``device`` (uploaded once per set_shifts)."""
        key = str(device)
        if key not in self._device_words:
            self._device_words[key] = self.words.to(device)
        return self._device_words[key]

    def tensors(self):
        """Per tensor (global offset, O, I, R): what the numpy reference reads."""
        return [(o,) + tuple(v.view) for o, v in zip(self.layout.offsets, self.views)]
