"""Inputs of the temporal-gate tests (tests/test_graph_gate.py on the CPU, tests/test_gpu_graph_gate.py on the GPU): camera
ids, start frames and the gap of every case, with the length of its gated list -- TEST INFRASTRUCTURE."""
import functools

import numpy as np
import torch

import gate_ref
import graph_cases


def _starts(n, high, seed):
    return torch.randint(0, high, (n,), generator=torch.Generator().manual_seed(seed)).numpy()


# nine nodes: cameras A = {0, 1, 2}, B = {3, 4}, C = {5, 6, 7, 8}
NINE_CAMS = np.repeat(np.array([1, 2, 3]), (3, 2, 4))
NINE_STARTS = np.array([0, 100, 200, 50, 150, 100, 199, 300, 1000])
NINE_PAIRS = {(0, 3), (1, 3), (1, 4), (1, 5), (1, 6), (2, 4), (2, 6), (3, 5), (4, 5), (4, 6)}    # kept at max_gap = 100
NINE_NOTHING = np.array([0, 100, 200, 50, 150, 101, 199, 300, 1000])                            # no two starts agree


def wave():             # out-degrees 71, 75 and 6: around a 64-wide wave; a one-node camera
    return np.repeat(np.array([0, 1, 2]), (5, 1, 70)), _starts(76, 1000, 31)


def interleaved():      # training order: the list's row order is not node order
    perm = torch.randperm(62, generator=torch.Generator().manual_seed(4)).numpy()
    return np.repeat(np.array([0, 1, 2]), (20, 17, 25))[perm], _starts(62, 1000, 32)


def sweeps():           # rows longer than one 256-wide sweep; 961 <= N <= 1920: the exact-fp32 Gram regime
    return np.repeat(np.array([0, 1, 2]), (300, 257, 543)), _starts(1100, 3000, 33)


def s02():
    return np.repeat(np.array([6, 7, 8, 9]), graph_cases.S02_GT_CAMS), _starts(450, 2110, 34)


# name -> (cams, starts, max_gap, length of the gated list)
COUNTS = {
    "nine": (NINE_CAMS, NINE_STARTS, 100, 20),
    "nine, whole span": (NINE_CAMS, NINE_STARTS, 1001, 52),
    "nine, nothing kept": (NINE_CAMS, NINE_NOTHING, 1, 0),
    "wave": (*wave(), 150, 274),
    "interleaved": (*interleaved(), 200, 878),
    "sweeps": (*sweeps(), 1200, 474368),
    "sweeps, tight gate": (*sweeps(), 2, 770),
    "s02": (*s02(), 300, 38606),
}


@functools.lru_cache(maxsize=None)
def dense_gate(name):
    """(dense edge_index of the case, its gated positions by the reference's loop); computed once, read only."""
    from oracle import graph_oracle
    cams, starts, gap, _ = COUNTS[name]
    ei = graph_oracle.topology(cams)
    return ei, gate_ref.select(starts, ei, gap)
