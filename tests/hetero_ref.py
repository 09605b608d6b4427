"""The two fed_hetero contracts of include/dls_hip.h restated in numpy float32: plain loops over
the clients, np.roll for the windows.  float32 arrays round every *, + and / once, which is
the contract.  ``tensors``: per tensor (global offset, O, I, R); ``slices[l]``: per tensor
(offset in level l's row, O_l, I_l, shO, shI) -- ``HeteroPlan.tensors()`` and ``.slices``."""
import numpy as np


def window(a, Ol, Il, shO, shI):
    """The level's [O_l, I_l, R] part of the global [O, I, R]: local j is global (shift + j) mod C."""
    return np.roll(a, (-shO, -shI), axis=(0, 1))[:Ol, :Il]


def extract(flat, tensors, level, level_P):
    """Level ``level``'s compact row of the global row: copies, zero padding."""
    row = np.zeros(level_P, flat.dtype)
    for (goff, O, I, R), (loff, Ol, Il, shO, shI) in zip(tensors, level):
        part = window(flat[goff:goff + O * I * R].reshape(O, I, R), Ol, Il, shO, shI)
        row[loff:loff + part.size] = part.ravel()
    return row


def scatter(row, tensors, level, P, fill=0):
    """The inverse of extract: (the row's values at their global places, who is held)."""
    out, held = np.full(P, fill, row.dtype), np.zeros(P, bool)
    for (goff, O, I, R), (loff, Ol, Il, shO, shI) in zip(tensors, level):
        full, mask = np.full((O, I, R), fill, row.dtype), np.zeros((O, I, R), bool)
        win = np.roll(full, (-shO, -shI), axis=(0, 1))
        win[:Ol, :Il] = row[loff:loff + Ol * Il * R].reshape(Ol, Il, R)
        out[goff:goff + O * I * R] = np.roll(win, (shO, shI), axis=(0, 1)).ravel()
        mwin = np.roll(mask, (-shO, -shI), axis=(0, 1))
        mwin[:Ol, :Il] = True
        held[goff:goff + O * I * R] = np.roll(mwin, (shO, shI), axis=(0, 1)).ravel()
    return out, held


def fedavg(rows, levels, weights, prev, tensors, slices, dtype=np.float32):
    """out per coordinate: acc = the chain of fl(w_k * u_k) over the clients that hold it, in
    the order given, the first assigning; den the same chain over w_k; out = fl(acc / den);
    prev's bits where nobody holds it; zero in the padding.  Also returns the member counts."""
    P = prev.size
    acc, den, count = np.zeros(P, dtype), np.zeros(P, dtype), np.zeros(P, np.int64)
    real = np.zeros(P, bool)
    for goff, O, I, R in tensors:
        real[goff:goff + O * I * R] = True
    with np.errstate(all="ignore"):
        for row, lvl, w in zip(rows, levels, weights):
            u, held = scatter(np.asarray(row, dtype), tensors, slices[lvl], P)
            term = u * dtype(w)
            first = held & (count == 0)
            acc = np.where(first, term, np.where(held, acc + term, acc))
            den = np.where(first, dtype(w), np.where(held, den + dtype(w), den))
            count += held
        out = np.where(count > 0, acc / np.where(count > 0, den, 1), prev.astype(dtype))
    if dtype is np.float32:  # prev's bits, not its value
        out = np.where(count > 0, out.view(np.uint32), prev.view(np.uint32)).view(np.float32)
    return np.where(real, out, dtype(0)), count
