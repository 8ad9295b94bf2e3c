"""What the front ends of the planners (leaders.py, failover.py) share: the marshalling of rows and weights for the C ABI and the
argument readers of their command lines."""
from __future__ import annotations

import argparse
import json
import re

import numpy as np

MAX_WEIGHT = 1 << 53   # weights above it are not exact as JSON doubles (the C++ reader): rejected, never rounded


def dense_rows(rows):
    """(r, flat, P, W): `rows` as a fresh C-ordered [P, W] uint16 array and the buffer handed to the library (one spare word when empty)."""
    r = np.array(rows, dtype=np.uint16, order="C")
    if r.ndim != 2:
        raise ValueError("rows must be a [P, width] array")
    P, W = r.shape
    return r, (r.reshape(-1) if r.size else np.zeros(1, dtype=np.uint16)), P, W


def weight_buffer(weight, P: int, min_gain):
    """The uint64 buffer of `weight` (one value per row, integers >= 0), min_gain checked beside it."""
    wt = np.asarray(weight).reshape(-1)
    if wt.shape != (P,):
        raise ValueError(f"weight must hold one value per row ({P}), got {wt.shape[0]}")
    if P and wt.dtype.kind not in "ui":
        raise ValueError("weights must be integers")
    if P and wt.dtype.kind == "i" and (wt < 0).any():
        raise ValueError("weights must be >= 0")
    if not 0 <= int(min_gain) < 1 << 64:
        raise ValueError("min_gain must be 0..2^64-1")
    return np.ascontiguousarray(wt, dtype=np.uint64) if P else np.zeros(1, dtype=np.uint64)


def count(text):   # as the C++ tools read a count: digits only
    if not re.fullmatch(r"[0-9]{1,9}", text):
        raise argparse.ArgumentTypeError("needs a value >= 0")
    return int(text)


def u64(text):
    if not re.fullmatch(r"[0-9]{1,20}", text) or int(text) >= 1 << 64:
        raise argparse.ArgumentTypeError("needs a value 0..2^64-1")
    return int(text)


def weight_arg(text):
    if not re.fullmatch(r"[0-9]{1,16}", text) or int(text) > MAX_WEIGHT:
        raise argparse.ArgumentTypeError("needs a value 0..2^53")
    return int(text)


def _racks(arg: str) -> dict:
    if ":" in arg and "{" not in arg and not arg.endswith(".json"):
        return {int(k): v for k, v in (kv.split(":") for kv in arg.split(",") if kv)}
    with open(arg) as f:
        return {int(k): str(v) for k, v in json.load(f).items()}
