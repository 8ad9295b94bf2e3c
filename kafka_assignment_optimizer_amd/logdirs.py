"""Log-dir balance: the replica moves between the log dirs of one broker that lower the peak of the bytes a dir stores
(kao_balance_logdirs).

    python -m kafka_assignment_optimizer_amd.logdirs --current current.json --log-dirs log-dirs.txt [--broker-list 0,1,2] \
        [--min-gain 1G] [--max-rounds N] [--dry-run] [--exchange] --out plan.json --report

Every other planner treats a broker as one disk.  A JBOD broker has several log dirs, Kafka places a new replica in the dir with the
fewest partitions, not the fewest bytes, and the broker dies on its fullest dir.  This one reads `kafka-log-dirs --describe` output
WITH its directories and moves replicas between the dirs of their own broker (an intra-broker move: disk to disk, no network) until
no single move closes a gap of more than --min-gain bytes.  The brokers are independent; each gets a deterministic descent with a
lower bound beside it: where peak_after == lower_bound on every broker the peaks are proven optimal.  The plan lists the partitions
with a moved replica, `replicas` as they are and a `log_dirs` list beside them ("any" for a slot that stays), which is what
kafka-reassign-partitions --execute takes.  With --exchange a broker that has no such move left goes on with exchanges of two replicas
between two of its dirs (kao_balance_logdirs_exchange) until no exchange closes a gap either: the peaks are never
higher and often lower, for more bytes copied; by bytes only, so not with the placement or the utilisation modes below.

With --plan FILE and / or --evacuate BROKER:DIR (repeatable) the replicas that have no dir yet get one (kao_place_logdirs, DESIGN.md
section 4p): those that the plan brings to a listed broker and those of a dir that is being emptied go, the largest first, to the
dir of their broker with the fewest bytes at that moment; --rebalance lets the residents move as well (the rounds above, in the same
call), --default-size N gives a size to an arrival that --log-dirs does not list.  The plan then lists the partitions of --plan and
those with a placed or moved replica, with the dir's name in the slot of such a replica.

With --utilisation, --capacities FILE or --default-capacity N the dirs have sizes and every mode above lowers the peak UTILISATION
L(d) / capacity(d) instead of the peak bytes (kao_balance_logdirs_capacity, kao_place_logdirs_capacity): the
answer for a broker whose volumes are unequal.  A usable dir takes its capacity from its entry in FILE ({"<brokerId>": {"<logDir>":
bytes}} or {"<brokerId>": bytes} for every dir of the broker; a value is a number or a string with K/M/G/T), else with --utilisation
from the totalBytes of the document when above 0 (Kafka >= 3.3), else from --default-capacity; a usable dir of a listed broker with
none is a usage error.  The plan has the same format; the report gains the utilisations in parts per million and the proof.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from .solver import STATUS_NAMES, _check

STAT_KEYS = ("brokers_moved", "rounds", "moves", "proposals", "launches", "stopped_by_max_rounds", "proven", "max_rounds_of_a_broker")
PER_BROKER_KEYS = ("peak_before", "peak_after", "lower_bound", "moved", "bytes_moved", "rounds")
# kao_balance_logdirs_exchange: rounds, moves and proposals count both kinds of round
X_STAT_KEYS = STAT_KEYS + ("exchange_rounds", "exchanges", "exchange_proposals", "brokers_lowered_by_exchange")
X_PER_BROKER_KEYS = PER_BROKER_KEYS + ("exchange_rounds", "exchanges")
# the capacity calls: the peaks and the bound are fractions {bytes, capacity}; proof: 0 gap, 1 bound met, 2 integrality test only
CAP_PER_BROKER_KEYS = ("peak_before", "cap_before", "peak_after", "cap_after", "lower_bound_num", "lower_bound_den", "moved", "bytes_moved", "rounds", "proof")
CAP_PLACE_PER_BROKER_KEYS = ("peak_before", "cap_before", "peak_after", "cap_after", "lower_bound_num", "lower_bound_den", "placed", "bytes_placed", "moved",
                             "bytes_moved", "rounds", "proof")


@dataclass
class LogDir:
    error: Optional[str]                                                        # non-null: the dir is offline and left out
    entries: List[Tuple[str, int, int, bool]] = field(default_factory=list)    # (topic, partition, size, isFuture)
    total_bytes: Optional[int] = None                                           # totalBytes / usableBytes of the volume (Kafka >= 3.3, KIP-827); None when absent or null
    usable_bytes: Optional[int] = None


@dataclass
class LogDirsResult:
    dir: np.ndarray          # [R] int32: the dir of every replica after the moves (the input with dry_run)
    n_moved: int             # replicas whose final dir differs from their input dir
    bytes_moved: int         # ... weighted by their sizes
    peak_before: int         # max_d L(d) of the input, over all dirs
    peak_after: int
    per_broker: np.ndarray   # [B, 6] uint64, see PER_BROKER_KEYS; [B, 8] with exchange=True, see X_PER_BROKER_KEYS
    status: str              # "OPTIMAL_PROVEN" (peak_after == lower_bound on every broker) | "FEASIBLE_BOUND_GAP"
    stats: np.ndarray        # int64[8], see STAT_KEYS / include/kao.h; int64[12] with exchange=True, see X_STAT_KEYS
    # with capacity= alone (else None): the fullest dir as {bytes, capacity}; peak_before / peak_after are then its bytes and
    # per_broker is [B, 10], see CAP_PER_BROKER_KEYS
    peak_before_frac: Optional[Tuple[int, int]] = None
    peak_after_frac: Optional[Tuple[int, int]] = None


def parse_log_dirs(doc_or_text) -> Dict[int, Dict[str, LogDir]]:
    """{broker id: {dir name: LogDir}} from the output of `kafka-log-dirs --describe` (text: the status lines before the JSON line are
    skipped; or the parsed JSON).  What waves.parse_sizes folds into one number per partition stays apart here: the directory, its
    error, the future replicas.  Partition names split at their last '-'; sizes are integers 0..2^53."""
    from .waves import _size_value
    doc = doc_or_text
    if isinstance(doc_or_text, (str, bytes)):
        text = doc_or_text.decode() if isinstance(doc_or_text, bytes) else doc_or_text
        try:
            doc = json.loads(text)
        except ValueError:
            doc = None
            for line in text.splitlines():
                if line.lstrip().startswith("{"):
                    doc = json.loads(line)
                    break
            if doc is None:
                raise ValueError("log-dirs: no JSON document found") from None
    if not isinstance(doc, dict) or not isinstance(doc.get("brokers"), list):
        raise ValueError('log-dirs: expected a "brokers" (kafka-log-dirs) document')
    out: Dict[int, Dict[str, LogDir]] = {}
    for br in doc["brokers"]:
        if isinstance(br.get("broker"), bool) or not isinstance(br.get("broker"), int):
            raise ValueError("log-dirs: broker entry without an integer id")
        b = int(br["broker"])
        if b in out:
            raise ValueError(f"log-dirs: broker {b} listed twice")
        dirs = out[b] = {}
        for ld in br.get("logDirs") or []:
            name = ld.get("logDir")
            if not isinstance(name, str):
                raise ValueError(f"log-dirs: broker {b}: log dir without a name")
            if name in dirs:
                raise ValueError(f"log-dirs: broker {b}: log dir {name} listed twice")
            err = ld.get("error")
            d = dirs[name] = LogDir(error=None if err is None else str(err))
            for attr, field_name in (("total_bytes", "totalBytes"), ("usable_bytes", "usableBytes")):
                if ld.get(field_name) is not None:
                    setattr(d, attr, _size_value(ld[field_name], f"log-dirs: broker {b}: {name}: {field_name}"))
            for e in ld.get("partitions") or []:
                pname = e.get("partition")
                if not isinstance(pname, str):
                    raise ValueError("log-dirs: log-dir entry without a partition name")
                topic, dash, idx = pname.rpartition("-")
                if not dash or not topic or not idx.isdigit() or len(idx) > 9:
                    raise ValueError(f"log-dirs: partition name '{pname}' is not <topic>-<partition>")
                d.entries.append((topic, int(idx), _size_value(e.get("size"), "log-dirs: " + pname), e.get("isFuture") is True))
    return out


def _table_of(log_dirs) -> Dict[int, Dict[str, LogDir]]:
    return log_dirs if isinstance(log_dirs, dict) and "brokers" not in log_dirs else parse_log_dirs(log_dirs)   # a parse_log_dirs table as it is


def _capacity_buffer(capacity, n_dirs: int) -> np.ndarray:
    """cap[] of a capacity call as a uint64 buffer (one spare word for a call without dirs): one integer >= 1 per dir, the sum below
    2^62; a ValueError otherwise."""
    if isinstance(capacity, np.ndarray) and capacity.dtype.kind in "ui" and capacity.dtype != np.bool_:   # no Python loop over an integer array
        cp = capacity.reshape(-1)
        if cp.shape[0] != max(n_dirs, 0):
            raise ValueError(f"capacity must hold one value per dir ({n_dirs}), got {cp.shape[0]}")
        if cp.size and int(cp.min()) < 1:
            raise ValueError("capacity: every capacity must be an integer >= 1")
        u = np.ascontiguousarray(cp, dtype=np.uint64)
        if (int((u >> np.uint64(32)).sum()) << 32) + int((u & np.uint64(0xFFFFFFFF)).sum()) >= 1 << 62:   # the two halves: no sum passes 64 bits
            raise ValueError("capacity: the capacities sum to 2^62 or more")
        return u if u.size else np.ones(1, dtype=np.uint64)
    values = list(np.asarray(capacity, dtype=object).reshape(-1))
    if len(values) != max(n_dirs, 0):
        raise ValueError(f"capacity must hold one value per dir ({n_dirs}), got {len(values)}")
    if any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < 1 for v in values):
        raise ValueError("capacity: every capacity must be an integer >= 1")
    if sum(int(v) for v in values) >= 1 << 62:
        raise ValueError("capacity: the capacities sum to 2^62 or more")
    return np.array([int(v) for v in values] or [1], dtype=np.uint64)


@dataclass
class _Arrays:
    """The arrays of a call, checked: dir_start and the result's copy of dir, and the buffers the library reads (one spare word where an
    array is empty; base and broker None when not given)."""
    ds: np.ndarray
    d: np.ndarray
    dbuf: np.ndarray
    sbuf: np.ndarray
    bbuf: Optional[np.ndarray]
    rbuf: Optional[np.ndarray]


def _checked_arrays(dir_start, dir, size, base, min_gain, broker=None) -> _Arrays:
    ds = np.ascontiguousarray(np.asarray(dir_start).reshape(-1), dtype=np.int32)
    if ds.shape[0] < 2:
        raise ValueError("dir_start must hold n_brokers + 1 values, n_brokers >= 1")
    d = np.array(np.asarray(dir).reshape(-1), dtype=np.int32, order="C")
    R = d.shape[0]
    rbuf = None
    if broker is not None:
        br = np.asarray(broker).reshape(-1)
        if br.shape != (R,):
            raise ValueError(f"broker must hold one value per replica ({R}), got {br.shape[0]}")
        if R and br.dtype.kind not in "ui":
            raise ValueError("brokers must be integers")
        rbuf = np.ascontiguousarray(br, dtype=np.int32) if R else np.zeros(1, dtype=np.int32)
    sz = np.asarray(size).reshape(-1)
    if sz.shape != (R,):
        raise ValueError(f"size must hold one value per replica ({R}), got {sz.shape[0]}")
    if R and (sz.dtype.kind not in "ui" or (sz.dtype.kind == "i" and (sz < 0).any())):
        raise ValueError("sizes must be integers >= 0")
    if isinstance(min_gain, bool) or not 0 <= int(min_gain) < 1 << 64:
        raise ValueError("min_gain must be 0..2^64-1")
    bbuf = None
    if base is not None:
        bs = np.asarray(base).reshape(-1)
        if bs.shape != (max(int(ds[-1]), 0),):
            raise ValueError(f"base must hold one value per dir ({int(ds[-1])}), got {bs.shape[0]}")
        if bs.size and (bs.dtype.kind not in "ui" or (bs.dtype.kind == "i" and (bs < 0).any())):
            raise ValueError("bases must be integers >= 0")
        bbuf = np.ascontiguousarray(bs, dtype=np.uint64) if bs.size else np.zeros(1, dtype=np.uint64)
    return _Arrays(ds=ds, d=d, dbuf=d if R else np.zeros(1, dtype=np.int32), sbuf=np.ascontiguousarray(sz, dtype=np.uint64) if R else np.zeros(1, dtype=np.uint64),
                   bbuf=bbuf, rbuf=rbuf)


def _call(entry: str, a: _Arrays, capacity, options: Sequence[int], n_outs: int, row: int, n_stats: int):
    """entry(n_brokers, dir_start, base, [cap,] n_replicas, [broker,] dir, size, *options, n_outs pairs {int32 *count, uint64 *bytes},
    peak_before, peak_after, per_broker[B, row], status, stats[n_stats]), checked.  Returns the counts and bytes in that order and the
    fields that every result class has.  A call by bytes writes the first word of a peak alone."""
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    B, R = a.ds.shape[0] - 1, a.d.shape[0]
    cbuf = None if capacity is None else _capacity_buffer(capacity, int(a.ds[-1]))
    per, stats, peaks, status = np.zeros((B, row), dtype=np.uint64), np.zeros(n_stats, dtype=np.int64), np.zeros((2, 2), dtype=np.uint64), C.c_int32(0)
    outs = [x for _ in range(n_outs) for x in (C.c_int32(0), C.c_uint64(0))]
    args = [B, a.ds.ctypes.data_as(i32p), None if a.bbuf is None else a.bbuf.ctypes.data_as(u64p)]
    args += [] if cbuf is None else [cbuf.ctypes.data_as(u64p)]
    args += [R] + ([] if a.rbuf is None else [a.rbuf.ctypes.data_as(i32p)]) + [a.dbuf.ctypes.data_as(i32p), a.sbuf.ctypes.data_as(u64p)]
    args += [int(o) for o in options] + [C.byref(x) for x in outs]
    args += [peaks[0].ctypes.data_as(u64p), peaks[1].ctypes.data_as(u64p), per.ctypes.data_as(u64p), C.byref(status), stats.ctypes.data_as(C.POINTER(C.c_int64))]
    _check(getattr(_ffi.load(), entry)(*args), entry)
    rest = dict(dir=a.d, peak_before=int(peaks[0, 0]), peak_after=int(peaks[1, 0]), per_broker=per, status=STATUS_NAMES[int(status.value)], stats=stats)
    if cbuf is not None:
        rest.update(peak_before_frac=(int(peaks[0, 0]), int(peaks[0, 1])), peak_after_frac=(int(peaks[1, 0]), int(peaks[1, 1])))
    return [int(x.value) for x in outs], rest


def balance_logdirs_arrays(dir_start, dir, size, base=None, min_gain: int = 0, max_rounds: int = 0, dry_run: bool = False, capacity=None,
                           exchange: bool = False) -> LogDirsResult:
    """kao_balance_logdirs on arrays: broker b owns the dirs dir_start[b] .. dir_start[b+1]-1, replica r sits in dir[r] with size[r]
    bytes, dir d carries base[d] bytes that never move.  capacity[d] >= 1 (the bytes of disk behind dir d) selects
    kao_balance_logdirs_capacity: the descent lowers L(d) / capacity[d], the result carries fractions.  exchange=True selects
    kao_balance_logdirs_exchange (bytes only): exchange rounds follow when no move is left; per_broker is [B, 8], stats int64[12]."""
    if exchange and capacity is not None:
        raise ValueError("exchange moves are by bytes only: exchange=True cannot be combined with capacity")
    a = _checked_arrays(dir_start, dir, size, base, min_gain)
    entry, row, n_stats = ("kao_balance_logdirs_capacity", 10, 8) if capacity is not None else ("kao_balance_logdirs_exchange", 8, 12) if exchange \
        else ("kao_balance_logdirs", 6, 8)
    (n, moved), rest = _call(entry, a, capacity, (min_gain, max_rounds, bool(dry_run)), 1, row, n_stats)
    return LogDirsResult(n_moved=n, bytes_moved=moved, **rest)


PLACE_STAT_KEYS = ("brokers_placed", "brokers_moved", "rounds", "moves", "proposals", "launches", "stopped_by_max_rounds", "proven", "max_rounds_of_a_broker",
                   "max_homeless_of_a_broker")
PLACE_PER_BROKER_KEYS = ("peak_before", "peak_after", "lower_bound", "placed", "bytes_placed", "moved", "bytes_moved", "rounds")


@dataclass
class PlaceLogDirsResult:
    dir: np.ndarray          # [R] int32: the dir of every replica after the call (the input, homeless replicas at -1, with dry_run)
    n_placed: int            # homeless replicas, each given a dir
    bytes_placed: int
    n_moved: int             # residents whose final dir differs from their input dir
    bytes_moved: int
    peak_before: int         # max_d F(d): the input without the homeless replicas
    peak_after: int
    per_broker: np.ndarray   # [B, 8] uint64, see PLACE_PER_BROKER_KEYS
    status: str              # "OPTIMAL_PROVEN" (peak_after == lower_bound on every broker) | "FEASIBLE_BOUND_GAP"
    stats: np.ndarray        # int64[10], see PLACE_STAT_KEYS / include/kao.h
    # with capacity= alone (else None): the fullest dir as {bytes, capacity}; per_broker is then [B, 12], see CAP_PLACE_PER_BROKER_KEYS
    peak_before_frac: Optional[Tuple[int, int]] = None
    peak_after_frac: Optional[Tuple[int, int]] = None


def place_logdirs_arrays(dir_start, broker, dir, size, base=None, move_residents: bool = False, min_gain: int = 0, max_rounds: int = 0,
                         dry_run: bool = False, capacity=None) -> PlaceLogDirsResult:
    """kao_place_logdirs on arrays: replica r belongs to broker[r] and sits in dir[r], or is homeless (dir[r] == -1) and gets the
    lightest dir of its broker, the largest replica first; with move_residents the rounds of kao_balance_logdirs follow.
    capacity[d] >= 1 selects kao_place_logdirs_capacity: a homeless replica goes to the dir that is the least full with it, the
    rounds lower L(d) / capacity[d], the result carries fractions."""
    a = _checked_arrays(dir_start, dir, size, base, min_gain, broker)
    entry, row = ("kao_place_logdirs_capacity", 12) if capacity is not None else ("kao_place_logdirs", 8)
    (placed, pbytes, n, moved), rest = _call(entry, a, capacity, (bool(move_residents), min_gain, max_rounds, bool(dry_run)), 2, row, 10)
    return PlaceLogDirsResult(n_placed=placed, bytes_placed=pbytes, n_moved=n, bytes_moved=moved, **rest)


@dataclass
class LogDirsInput:
    """The documents as the arrays of the call (the mapping is that of cli/kao-logdirs, so both write the same bytes)."""
    broker_ids: List[int]                 # dense broker index -> broker id
    dir_names: List[List[str]]            # per broker: its usable dirs, byte-wise ascending
    skipped: List[int]                    # per broker: dirs left out for their error
    dir_start: np.ndarray                 # [B + 1] int32
    base: np.ndarray                      # [n_dirs] uint64
    dir: np.ndarray                       # [R] int32
    size: np.ndarray                      # [R] uint64
    slots: List[Tuple[int, int]]          # per replica: (index into keys, slot of the row)
    keys: List[Tuple[str, int]]           # (topic, partition) ascending
    rows: List[List[int]]                 # per key: the replicas of --current as broker ids


def parse_input(current_doc: dict, log_dirs, broker_list: Optional[Sequence[int]] = None) -> LogDirsInput:
    """Brokers: those of broker_list in that order (default: every broker of the log-dirs document, ascending id); a broker outside
    the list is left alone.  Dirs: a broker's usable dirs (error null) byte-wise ascending by name.  Replicas: the partitions of the
    current document by (topic, partition), the slots of a row in order; a slot is a movable replica iff its broker is in the list
    and has a non-future entry for the partition in a usable dir, whose size it takes.  Every other entry of a usable dir (future
    replicas, partitions the current document does not hold, brokers outside the partition's row) adds its size to the dir's base.
    The same partition non-future twice on one broker is a ValueError.  The mapping is parse_place_input's without a plan and without
    an evacuation: every replica a resident of its broker, nothing stranded."""
    pi = parse_place_input(current_doc, log_dirs, None, (), broker_list)
    return LogDirsInput(**{f: getattr(pi, f) for f in LogDirsInput.__dataclass_fields__})


def dir_capacities(broker_ids: Sequence[int], dir_names: Sequence[Sequence[str]], table: Dict[int, Dict[str, LogDir]], capacity: Optional[dict] = None,
                   default_capacity: Optional[int] = None, use_total_bytes: bool = False) -> List[int]:
    """capacity[d] of every usable dir, in the order of the call's dirs.  Per dir: its entry in `capacity` ({broker id: {dir name:
    bytes}} or {broker id: bytes} for every dir of that broker; a value an integer or a string with K/M/G/T, as disk.capacity_of takes
    them), else with use_total_bytes the totalBytes of the document when above 0, else default_capacity; a dir with none is a
    ValueError.  Entries of brokers and dirs that the call does not hold are ignored."""
    from .waves import parse_bytes

    def value(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer, str)):
            raise ValueError(f"capacity of {what}: not a byte count: {v!r}")
        try:
            return parse_bytes(str(int(v)) if not isinstance(v, str) else v)
        except ValueError:
            raise ValueError(f"capacity of {what}: not a byte count: {v!r}") from None

    given: Dict[int, object] = {}
    for k, v in (capacity or {}).items():
        if isinstance(v, dict):
            given[int(k)] = {str(n): value(x, f"log dir {int(k)}:{n}") for n, x in v.items()}
        else:
            given[int(k)] = value(v, f"broker {int(k)}")
    out, missing = [], []
    for b, names in zip(broker_ids, dir_names):
        mine = given.get(int(b))
        for n in names:
            total = table.get(int(b), {}).get(n).total_bytes if use_total_bytes else None
            if isinstance(mine, dict) and n in mine:
                out.append(mine[n])
            elif mine is not None and not isinstance(mine, dict):
                out.append(mine)
            elif total:
                out.append(int(total))
            elif default_capacity is not None:
                out.append(int(default_capacity))
            else:
                missing.append(f"{int(b)}:{n}")
    if missing:
        raise ValueError("no capacity for log dirs " + ", ".join(missing[:5]) + (f" and {len(missing) - 5} more" if len(missing) > 5 else "")
                         + " (give them in --capacities, read totalBytes with --utilisation or set --default-capacity)")
    return out


def _ppm(num: int, den: int) -> int:
    return int(num) * 10 ** 6 // int(den)


def _capacity_warnings(broker_ids, dir_names, dir_start, base, capacity) -> List[str]:
    """One line per dir whose base alone exceeds its capacity."""
    out = []
    for i, b in enumerate(broker_ids):
        for li, n in enumerate(dir_names[i]):
            d = int(dir_start[i]) + li
            if int(base[d]) > int(capacity[d]):
                out.append(f"logdirs: warning: broker={b} dir={n} base={int(base[d])} exceeds capacity={int(capacity[d])}")
    return out


def _quoted(s: str) -> str:
    return '"' + s.replace("\\", "\\\\").replace('"', '\\"') + '"'


class _PlanDocument:
    """What LogDirsPlan and PlaceLogDirsPlan do with their entries."""

    def document(self) -> dict:
        """The reassignment document of the entries, each with its log_dirs (what kafka-reassign-partitions --execute takes)."""
        return {"version": 1, "partitions": [{"topic": t, "partition": p, "replicas": r, "log_dirs": d} for t, p, r, d in self.entries]}

    def text(self) -> str:
        """The document byte for byte as cli/kao-logdirs writes it."""
        rows = ['    {"topic":%s,"partition":%d,"replicas":[%s],"log_dirs":[%s]}' % (_quoted(t), p, ",".join(str(b) for b in r), ",".join(_quoted(x) for x in d))
                for t, p, r, d in self.entries]
        return '{"version":1,"partitions":[' + "".join(("\n" if i == 0 else ",\n") + r for i, r in enumerate(rows)) + "\n]}\n"


def _plan_entries(inp, new_dir: np.ndarray, planned: Sequence[bool], dry_run: bool) -> List[Tuple[str, int, List[int], List[str]]]:
    """The entries of a plan on a LogDirsInput or a PlaceInput: the planned partitions and those with a replica whose dir changed, in
    the order of the keys; the new dir's name in the slot of such a replica and "any" in every other.  None with dry_run."""
    if dry_run:
        return []
    flat = [n for names in inp.dir_names for n in names]
    lists: Dict[int, List[str]] = {k: ["any"] * len(inp.rows[k]) for k, p in enumerate(planned) if p}
    for r in np.nonzero(new_dir != inp.dir)[0]:
        k, j = inp.slots[int(r)]
        lists.setdefault(k, ["any"] * len(inp.rows[k]))[j] = flat[int(new_dir[r])]
    return [(inp.keys[k][0], inp.keys[k][1], list(inp.rows[k]), lists[k]) for k in sorted(lists)]


@dataclass
class LogDirsPlan(_PlanDocument):
    result: LogDirsResult
    input: LogDirsInput
    entries: List[Tuple[str, int, List[int], List[str]]] = field(default_factory=list)   # (topic, partition, replicas, log_dirs) of the partitions with a move
    capacity: Optional[List[int]] = None                                                  # per dir of the call, with capacities alone
    exchange: bool = False                                                                # the call was kao_balance_logdirs_exchange

    def report_lines(self) -> List[str]:
        return report_lines(self)


def plan_input(li: LogDirsInput, min_gain: int = 0, max_rounds: int = 0, dry_run: bool = False, capacity: Optional[Sequence[int]] = None,
               exchange: bool = False) -> LogDirsPlan:
    """kao_balance_logdirs on a LogDirsInput (kao_balance_logdirs_capacity with capacity, one value per dir of li;
    kao_balance_logdirs_exchange with exchange); the entries are the partitions with a moved replica (none with dry_run)."""
    res = balance_logdirs_arrays(li.dir_start, li.dir, li.size, li.base, min_gain, max_rounds, dry_run, **({} if capacity is None else {"capacity": capacity}),
                                 **({"exchange": True} if exchange else {}))
    return LogDirsPlan(result=res, input=li, entries=_plan_entries(li, res.dir, (), dry_run), capacity=None if capacity is None else [int(x) for x in capacity],
                       exchange=bool(exchange))


def balance_logdirs(current_doc: dict, log_dirs, *, broker_list: Optional[Sequence[int]] = None, min_gain: int = 0, max_rounds: int = 0,
                    dry_run: bool = False, capacity: Optional[dict] = None, default_capacity: Optional[int] = None,
                    use_total_bytes: bool = False, exchange: bool = False) -> LogDirsPlan:
    """kao_balance_logdirs on a reassignment document and the `kafka-log-dirs --describe` output of its cluster (text, parsed JSON, or
    the table of parse_log_dirs).  plan.document() is the reassignment document with its log_dirs lists.  Any of capacity,
    default_capacity and use_total_bytes gives the dirs their sizes (dir_capacities) and selects kao_balance_logdirs_capacity.
    exchange=True selects kao_balance_logdirs_exchange (bytes only: a ValueError together with capacities)."""
    if exchange and (capacity is not None or default_capacity is not None or use_total_bytes):
        raise ValueError("exchange moves are by bytes only: exchange=True cannot be combined with capacities")
    table = _table_of(log_dirs)
    li = parse_input(current_doc, table, broker_list)
    cap = None
    if capacity is not None or default_capacity is not None or use_total_bytes:
        cap = dir_capacities(li.broker_ids, li.dir_names, table, capacity, default_capacity, use_total_bytes)
    return plan_input(li, min_gain, max_rounds, dry_run, cap, exchange)


def _report_parts(plan, columns: Sequence[str]):
    """What the two reports share: the warning lines; per broker the text of its columns, the capacity words folded away ({peak_before,
    cap, peak_after, cap, bound num, den, <the other columns>, proof} with capacities), and the ppm tail of its line; bytes_total; the
    ppm tail of the call's line."""
    res, inp = plan.result, plan.input
    by_cap = res.peak_after_frac is not None
    warnings = _capacity_warnings(inp.broker_ids, inp.dir_names, inp.dir_start, inp.base, plan.capacity) if by_cap else []
    cols, tails = [], []
    for row in res.per_broker:
        p = [int(x) for x in row]
        tails.append(f" peak_before_ppm={_ppm(p[0], p[1])} peak_after_ppm={_ppm(p[2], p[3])} lower_bound_ppm={_ppm(p[4], p[5])} proof={p[-1]}" if by_cap else "")
        cols.append(" ".join(f"{k}={v}" for k, v in zip(columns, p[0:6:2] + p[6:-1] if by_cap else p)))
    total = sum(int(x) for x in inp.size) + sum(int(x) for x in inp.base)
    return warnings, cols, tails, total, f" peak_before_ppm={_ppm(*res.peak_before_frac)} peak_after_ppm={_ppm(*res.peak_after_frac)}" if by_cap else ""


def report_lines(plan: LogDirsPlan) -> List[str]:
    """The --report text, line for line as cli/kao-logdirs prints it: one line per broker, one for the call."""
    res, li = plan.result, plan.input
    per_replicas = np.bincount(np.searchsorted(li.dir_start, li.dir, side="right") - 1, minlength=len(li.broker_ids)) if len(li.dir) else [0] * len(li.broker_ids)
    out, cols, tails, total, call_tail = _report_parts(plan, X_PER_BROKER_KEYS if plan.exchange else PER_BROKER_KEYS)
    for i, b in enumerate(li.broker_ids):
        out.append(f"logdirs: broker={b} dirs={len(li.dir_names[i])} skipped_dirs={li.skipped[i]} replicas={int(per_replicas[i])} {cols[i]}{tails[i]}")
    out.append(f"logdirs: status={res.status} brokers={len(li.broker_ids)} dirs={int(li.dir_start[-1])} skipped_dirs={sum(li.skipped)} replicas={len(li.dir)} "
               f"peak_before={res.peak_before} peak_after={res.peak_after} replicas_moved={res.n_moved} bytes_moved={res.bytes_moved} bytes_total={total} "
               + " ".join(f"{k}={int(v)}" for k, v in zip(X_STAT_KEYS if plan.exchange else STAT_KEYS, res.stats)) + call_tail)
    return out


# ---- placement: log dirs for the replicas a plan brings to a broker and for those of an evacuated dir ----------
@dataclass
class PlaceInput:
    """The documents as the arrays of kao_place_logdirs (the mapping is that of cli/kao-logdirs --plan / --evacuate)."""
    broker_ids: List[int]                 # dense broker index -> broker id
    dir_names: List[List[str]]            # per broker: its usable dirs without the evacuated ones, byte-wise ascending
    skipped: List[int]                    # per broker: dirs left out for their error
    evacuated: List[int]                  # per broker: dirs that are being evacuated
    stranded: List[int]                   # per broker: bytes of the entries of its evacuated dirs that are not planned
    dir_start: np.ndarray                 # [B + 1] int32
    base: np.ndarray                      # [n_dirs] uint64
    broker: np.ndarray                    # [R] int32
    dir: np.ndarray                       # [R] int32, -1 = homeless
    size: np.ndarray                      # [R] uint64
    slots: List[Tuple[int, int]]          # per replica: (index into keys, slot of the row)
    keys: List[Tuple[str, int]]           # (topic, partition) ascending
    rows: List[List[int]]                 # per key: the plan's row where there is one, else the row of --current
    planned: List[bool]                   # per key: the plan lists it


def parse_place_input(current_doc: dict, log_dirs, plan_doc: Optional[dict] = None, evacuate: Sequence[Tuple[int, str]] = (),
                      broker_list: Optional[Sequence[int]] = None, default_size: Optional[int] = None) -> PlaceInput:
    """parse_input's mapping with a plan and evacuations.  The plan is a reassignment document for a subset of the partitions of the
    current one; for a planned partition its row decides.  A broker of the row that the current row lacks gets an ARRIVAL: a homeless
    replica whose size is the largest non-future size of the partition in the whole log-dirs document (default_size without one),
    provided the broker is in the list and has a usable dir.  A broker of the current row that the plan's row lacks is a DEPARTURE:
    its entry counts neither as a replica nor as base (the result is made for the end state; Kafka keeps the old copy until the new
    one is in sync).  An evacuated dir leaves its broker's dir list; its non-future entries of partitions whose row still holds the
    broker become homeless there, its other entries are stranded: neither planned nor counted."""
    from .waves import _entries
    table = _table_of(log_dirs)
    ids = sorted(table) if broker_list is None else [int(b) for b in broker_list]
    if not ids:
        raise ValueError("empty broker list")
    if len(set(ids)) != len(ids):
        raise ValueError("duplicate id in broker list")
    dense = {b: i for i, b in enumerate(ids)}
    by_key = _entries(current_doc, "current")
    plan = _entries(plan_doc, "plan") if plan_doc is not None else {}
    for key, row in plan.items():
        if key not in by_key:
            raise ValueError(f"plan: partition {key[0]}-{key[1]} is not in the current assignment")
        if len(set(row)) != len(row):
            raise ValueError(f"plan: partition {key[0]}-{key[1]} lists a broker twice")
    keys = sorted(by_key, key=lambda k: (k[0].encode(), k[1]))
    out_of: List[set] = [set() for _ in ids]
    for b, name in evacuate:
        i = dense.get(int(b))
        d = table.get(int(b), {}).get(name) if i is not None else None
        if d is None or d.error is not None:
            raise ValueError(f"evacuate: {b}:{name} is not a usable log dir of a listed broker")
        out_of[i].add(name)
    psize: Dict[Tuple[str, int], int] = {}   # the largest non-future size of a partition anywhere: the size of an arrival
    for dirs in table.values():
        for d in dirs.values():
            for topic, part, sz, fut in d.entries:
                if not fut:
                    psize[(topic, part)] = max(psize.get((topic, part), 0), sz)
    names, skipped, dir_start = [], [], [0]
    where: List[Dict[Tuple[str, int], Tuple[int, int]]] = []   # per broker: partition -> (global dir, size) of its non-future entry in a dir that stays
    leaving: List[Dict[Tuple[str, int], int]] = []             # ... -> size of its non-future entry in an evacuated dir
    for i, b in enumerate(ids):
        dirs = table.get(b, {})
        usable = sorted((n for n, d in dirs.items() if d.error is None), key=lambda n: n.encode())
        stay = [n for n in usable if n not in out_of[i]]
        if out_of[i] and not stay:
            raise ValueError(f"evacuate: broker {b} is left without a usable log dir")
        names.append(stay)
        skipped.append(len(dirs) - len(usable))
        at: Dict[Tuple[str, int], Tuple[int, int]] = {}
        gone: Dict[Tuple[str, int], int] = {}
        for n in usable:
            for topic, part, sz, fut in dirs[n].entries:
                if fut:
                    continue
                if (topic, part) in at or (topic, part) in gone:
                    raise ValueError(f"log-dirs: broker {b} holds partition {topic}-{part} twice")
                if n in out_of[i]:
                    gone[(topic, part)] = sz
                else:
                    at[(topic, part)] = (dir_start[-1] + stay.index(n), sz)
        where.append(at)
        leaving.append(gone)
        dir_start.append(dir_start[-1] + len(stay))
    rbroker, rdir, rsize, slots, claimed, rescued, departed = [], [], [], [], set(), set(), set()
    rows = [plan.get(k, by_key[k]) for k in keys]
    for k, key in enumerate(keys):
        was = set(by_key[key])
        for x in was - set(rows[k]):
            if x in dense:
                departed.add((dense[x], key))
        for j, x in enumerate(rows[k]):
            i = dense.get(x)
            if i is None:
                continue
            if key in leaving[i]:                       # its dir is being evacuated
                d, sz = -1, leaving[i][key]
                rescued.add((i, key))
            elif x in was:
                if key not in where[i]:
                    continue
                d, sz = where[i][key]
                claimed.add((i, key))
            else:                                       # an arrival
                if not names[i]:
                    continue
                if key in psize:
                    d, sz = -1, psize[key]
                elif default_size is not None:
                    d, sz = -1, int(default_size)
                else:
                    raise ValueError(f"log-dirs: no size for partition {key[0]}-{key[1]}, which the plan brings to broker {x} (give a default size)")
            rbroker.append(i)
            rdir.append(d)
            rsize.append(sz)
            slots.append((k, j))
    base = [0] * dir_start[-1]
    stranded = [0] * len(ids)
    for i, b in enumerate(ids):
        for li, n in enumerate(names[i]):
            for topic, part, sz, fut in table[b][n].entries:
                if not fut and (i, (topic, part)) in departed:
                    continue
                if fut or (i, (topic, part)) not in claimed:
                    base[dir_start[i] + li] += sz
        for n in out_of[i]:
            for topic, part, sz, fut in table[b][n].entries:
                if fut or (i, (topic, part)) not in rescued:
                    stranded[i] += sz
    return PlaceInput(broker_ids=ids, dir_names=names, skipped=skipped, evacuated=[len(s) for s in out_of], stranded=stranded,
                      dir_start=np.asarray(dir_start, dtype=np.int32), base=np.asarray(base, dtype=np.uint64).reshape(-1),
                      broker=np.asarray(rbroker, dtype=np.int32).reshape(-1), dir=np.asarray(rdir, dtype=np.int32).reshape(-1),
                      size=np.asarray(rsize, dtype=np.uint64).reshape(-1), slots=slots, keys=keys, rows=rows, planned=[k in plan for k in keys])


@dataclass
class PlaceLogDirsPlan(_PlanDocument):
    result: PlaceLogDirsResult
    input: PlaceInput
    entries: List[Tuple[str, int, List[int], List[str]]] = field(default_factory=list)   # (topic, partition, replicas, log_dirs) of the plan's partitions and those with a placed or moved replica
    capacity: Optional[List[int]] = None                                                  # per dir of the call, with capacities alone

    def report_lines(self) -> List[str]:
        return place_report_lines(self)


def place_input(pi: PlaceInput, rebalance: bool = False, min_gain: int = 0, max_rounds: int = 0, dry_run: bool = False,
                capacity: Optional[Sequence[int]] = None) -> PlaceLogDirsPlan:
    """kao_place_logdirs on a PlaceInput (kao_place_logdirs_capacity with capacity, one value per dir of pi); the entries are the
    partitions of the plan and those with a placed or moved replica, the dir's name in the slot of such a replica and "any" in every
    other (no entry with dry_run)."""
    res = place_logdirs_arrays(pi.dir_start, pi.broker, pi.dir, pi.size, pi.base, rebalance, min_gain, max_rounds, dry_run,
                               **({} if capacity is None else {"capacity": capacity}))
    return PlaceLogDirsPlan(result=res, input=pi, entries=_plan_entries(pi, res.dir, pi.planned, dry_run), capacity=None if capacity is None else [int(x) for x in capacity])


def place_logdirs(current_doc: dict, log_dirs, plan_doc: Optional[dict] = None, evacuate: Sequence[Tuple[int, str]] = (),
                  broker_list: Optional[Sequence[int]] = None, rebalance: bool = False, min_gain: int = 0, max_rounds: int = 0,
                  default_size: Optional[int] = None, dry_run: bool = False, capacity: Optional[dict] = None, default_capacity: Optional[int] = None,
                  use_total_bytes: bool = False) -> PlaceLogDirsPlan:
    """kao_place_logdirs on a reassignment document, the `kafka-log-dirs --describe` output of its cluster, a plan for some of its
    partitions and a list of (broker id, dir name) to evacuate: every replica the plan brings to a listed broker and every replica
    of an evacuated dir gets a dir by name; with rebalance the residents may move as well (the rounds of balance_logdirs).  Any of
    capacity, default_capacity and use_total_bytes gives the dirs that stay their sizes (dir_capacities) and selects
    kao_place_logdirs_capacity."""
    table = _table_of(log_dirs)
    pi = parse_place_input(current_doc, table, plan_doc, evacuate, broker_list, default_size)
    cap = None
    if capacity is not None or default_capacity is not None or use_total_bytes:
        cap = dir_capacities(pi.broker_ids, pi.dir_names, table, capacity, default_capacity, use_total_bytes)
    return place_input(pi, rebalance, min_gain, max_rounds, dry_run, cap)


def place_report_lines(plan: PlaceLogDirsPlan) -> List[str]:
    """The --report text of a placement, line for line as cli/kao-logdirs prints it: one line per broker, one for the call."""
    res, pi = plan.result, plan.input
    B = len(pi.broker_ids)
    homeless = np.bincount(pi.broker[pi.dir < 0], minlength=B) if len(pi.dir) else np.zeros(B, dtype=np.int64)
    residents = np.bincount(pi.broker[pi.dir >= 0], minlength=B) if len(pi.dir) else np.zeros(B, dtype=np.int64)
    out, cols, tails, total, call_tail = _report_parts(plan, PLACE_PER_BROKER_KEYS)
    for i, b in enumerate(pi.broker_ids):
        out.append(f"logdirs: broker={b} dirs={len(pi.dir_names[i])} skipped_dirs={pi.skipped[i]} evacuated_dirs={pi.evacuated[i]} "
                   f"replicas={int(residents[i] + homeless[i])} residents={int(residents[i])} homeless={int(homeless[i])} {cols[i]} "
                   f"stranded_bytes={pi.stranded[i]}{tails[i]}")
    out.append(f"logdirs: status={res.status} brokers={B} dirs={int(pi.dir_start[-1])} skipped_dirs={sum(pi.skipped)} evacuated_dirs={sum(pi.evacuated)} "
               f"replicas={len(pi.dir)} residents={int(residents.sum())} homeless={int(homeless.sum())} peak_before={res.peak_before} peak_after={res.peak_after} "
               f"replicas_placed={res.n_placed} bytes_placed={res.bytes_placed} replicas_moved={res.n_moved} bytes_moved={res.bytes_moved} bytes_total={total} "
               f"stranded_bytes={sum(pi.stranded)} " + " ".join(f"{k}={int(v)}" for k, v in zip(PLACE_STAT_KEYS, res.stats)) + call_tail)
    return out


def _capacity_file(path: str) -> dict:
    """--capacities: a JSON file {"<brokerId>": {"<logDir>": bytes}} or {"<brokerId>": bytes}; the values as dir_capacities takes them."""
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict):
        raise ValueError('capacities file must be a JSON object {"<brokerId>": {"<logDir>": bytes} | bytes}')
    out = {}
    for k, v in doc.items():
        if not k.isdigit():
            raise ValueError(f"capacity of broker {k}: not a broker id")
        out[int(k)] = v
    return out


def main(argv=None) -> int:
    """Python twin of cli/kao-logdirs: same flags, same bytes, same exit status (0 ok, 1 error, 2 usage)."""
    from ._plan_args import count
    from .waves import parse_bytes
    ap = argparse.ArgumentParser(prog="kao-logdirs", description="replica moves between the log dirs of a broker that lower the peak bytes per dir")
    ap.add_argument("--current", required=True, help="reassignment JSON of the cluster as it is")
    ap.add_argument("--log-dirs", required=True, help="kafka-log-dirs --describe output")
    ap.add_argument("--broker-list", default=None, help="brokers to balance, CSV (default: every broker of --log-dirs)")
    ap.add_argument("--min-gain", default=None, help="move only to close a gap of more than N bytes (N, or N with K/M/G/T)")
    ap.add_argument("--max-rounds", type=count, default=0, help="stop every broker after N rounds")
    ap.add_argument("--dry-run", action="store_true", help="report only: the plan stays empty")
    ap.add_argument("--plan", default=None, help="reassignment JSON for some partitions of --current: its arrivals get a log dir")
    ap.add_argument("--evacuate", action="append", default=[], metavar="BROKER:DIR", help="empty this log dir into the broker's others (repeatable)")
    ap.add_argument("--rebalance", action="store_true", help="with --plan / --evacuate: the resident replicas may move as well")
    ap.add_argument("--default-size", default=None, help="with --plan / --evacuate: size of an arrival that --log-dirs does not list (N, or N with K/M/G/T)")
    ap.add_argument("--utilisation", action="store_true", help="lower the peak utilisation: a dir's capacity is the totalBytes of --log-dirs (Kafka >= 3.3)")
    ap.add_argument("--capacities", default=None, help='{"<brokerId>": {"<logDir>": bytes} | bytes} JSON file: lower the peak utilisation')
    ap.add_argument("--default-capacity", default=None, help="bytes of disk of the dirs that have no other capacity (N, or N with K/M/G/T)")
    ap.add_argument("--exchange", action="store_true", help="exchange two replicas of two dirs where no single move is left (bytes only)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    min_gain, default_size, evacuate = 0, None, []
    by_capacity, cap_table, default_capacity = a.utilisation or a.capacities is not None or a.default_capacity is not None, None, None
    placing = a.plan is not None or bool(a.evacuate)
    if (a.rebalance or a.default_size is not None) and not placing:
        ap.error("--rebalance and --default-size need --plan or --evacuate")
    if a.exchange and (placing or by_capacity):
        ap.error("--exchange cannot be combined with --utilisation, --capacities, --default-capacity, --plan, --evacuate or --rebalance")
    try:
        if a.min_gain is not None:
            min_gain = parse_bytes(a.min_gain)
        if a.default_size is not None:
            default_size = parse_bytes(a.default_size)
        for item in a.evacuate:
            b, colon, name = item.partition(":")
            if not colon or not name or not (b[1:] if b.startswith("-") else b).isdigit() or len(b) > 10:
                raise ValueError("--evacuate needs BROKER:DIR")
            evacuate.append((int(b), name))
        if a.default_capacity is not None:
            try:
                default_capacity = parse_bytes(a.default_capacity)
            except ValueError:
                raise ValueError("--default-capacity needs a byte count (N, or N with K/M/G/T)") from None
        if a.capacities is not None:
            try:
                cap_table = _capacity_file(a.capacities)
                dir_capacities([], [], {}, cap_table)   # its values, before any document is read
            except (OSError, ValueError) as e:
                raise ValueError(f"--capacities: {e}")
    except ValueError as e:
        ap.error(str(e))

    try:
        with open(a.current) as f:
            doc = json.load(f)
        with open(a.log_dirs) as f:
            text = f.read()
        ids = None if a.broker_list is None else [int(b) for b in a.broker_list.split(",") if b]
        from .solver import init
        plan_doc = None
        if a.plan is not None:
            with open(a.plan) as f:
                plan_doc = json.load(f)
        table = parse_log_dirs(text)
        inp = parse_place_input(doc, table, plan_doc, evacuate, ids, default_size) if placing else parse_input(doc, table, ids)   # input errors before the device is touched
        cap = None
        if by_capacity:
            try:
                cap = dir_capacities(inp.broker_ids, inp.dir_names, table, cap_table, default_capacity, a.utilisation)
            except ValueError as e:   # a usable dir without a capacity is a usage error
                ap.error(str(e))
        init(a.device)
        plan = place_input(inp, a.rebalance, min_gain, a.max_rounds, a.dry_run, cap) if placing else plan_input(inp, min_gain, a.max_rounds, a.dry_run, cap, a.exchange)
        if a.report:
            for line in plan.report_lines():
                print(line, file=sys.stderr)
        with open(a.out, "w") as f:
            f.write(plan.text())
    except Exception as e:  # noqa: BLE001 -- reported, exit status 1
        print(f"kao-logdirs: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
