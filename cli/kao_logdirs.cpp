// kao-logdirs -- log-dir balance: the replica moves between the log dirs of one broker that lower the peak of the bytes a dir stores
// (kao_balance_logdirs).
//
//   kao-logdirs --current current.json --log-dirs log-dirs.txt [--broker-list a,b,..] [--min-gain BYTES] [--max-rounds N] [--dry-run]
//               --out plan.json [--report] [--device D]
//
// Every other planner treats a broker as one disk.  A JBOD broker has several log dirs, Kafka places a new replica in the dir with
// the fewest partitions, not the fewest bytes, and the broker dies on its fullest dir.  This tool reads `kafka-log-dirs --describe`
// output WITH its directories and moves replicas between the dirs of their own broker (disk to disk, no network) until no single
// move closes a gap of more than --min-gain bytes (N, or N with K/M/G/T).
// From the documents to the arrays of the call:
//   brokers   those of --broker-list in that order (default: every broker of --log-dirs, ascending id); one outside it is left alone;
//   dirs      a broker's dirs byte-wise ascending by name; a dir whose "error" is non-null is left out (no destination, its entries
//             ignored, counted in the report);
//   replicas  the partitions of --current by (topic, partition), the slots of a row in order; a slot is a movable replica iff its
//             broker is in the list and has a non-future entry for the partition in a usable dir, whose size it takes;
//   base      every other entry of a usable dir adds its size to the bytes of that dir that never move: future replicas,
//             partitions --current does not hold, brokers that are not in the partition's row.
// The same partition non-future twice on one broker is an error.  The plan lists the partitions with a moved replica: "replicas" is
// the row of --current, "log_dirs" has the same length, the new dir's name for a moved slot and "any" for every other: what
// kafka-reassign-partitions --execute takes for an intra-broker move.  --dry-run reports and leaves the plan empty.  --report prints
// one line per broker and one for the call.  All computation happens in libkao.so on the GPU.
// With --exchange a broker that has no such move left goes on with exchanges of two replicas between two of its dirs until no
// exchange closes a gap of more than --min-gain either (kao_balance_logdirs_exchange); the report gains
// exchange_rounds and exchanges per broker and four counters for the call.  By bytes only: a usage error together with --plan,
// --evacuate, --rebalance, --utilisation, --capacities or --default-capacity.
//
// With --plan and / or --evacuate the tool gives log dirs to replicas that have none yet (kao_place_logdirs):
//   kao-logdirs --current current.json --log-dirs log-dirs.txt [--plan plan.json] [--evacuate BROKER:DIR]... [--rebalance]
//               [--default-size BYTES] [--broker-list a,b,..] [--min-gain BYTES] [--max-rounds N] [--dry-run] --out plan.json [--report]
//   --plan      a reassignment document for some partitions of --current; for a planned partition its row decides.  A broker of the
//               row that the current row lacks gets an ARRIVAL, a homeless replica of the size of the largest non-future entry of the
//               partition anywhere in --log-dirs (--default-size without one, else an error), if the broker is in the list and has
//               a usable dir; otherwise the slot stays "any".  A broker of the current row that the plan's row lacks is a DEPARTURE:
//               its entry is neither a replica nor base (the result is made for the end state; Kafka keeps the old copy until the
//               new one is in sync);
//   --evacuate  BROKER:DIR, split at the first ':', repeatable: the dir leaves the broker's dir list, its non-future entries of
//               partitions whose row still holds the broker become homeless on that broker, its other entries are stranded (neither
//               planned nor counted; reported as stranded_bytes);
//   --rebalance the resident replicas may move as well: the rounds of the balance run after the placement.
// Every homeless replica goes to the dir with the fewest bytes at that moment, the largest replica first.  The plan lists the
// partitions of --plan and those with a placed or moved replica: "replicas" is the plan's row where there is one, else the row of
// --current; "log_dirs" names the dir of a placed or moved slot and says "any" for every other.
// With --utilisation, --capacities FILE or --default-capacity BYTES the dirs have sizes, and every mode above lowers the peak
// UTILISATION L(d) / capacity(d) instead of the peak bytes (kao_balance_logdirs_capacity, kao_place_logdirs_capacity, DESIGN.md
// section 4r).  A usable dir takes its capacity from its entry in FILE ({"<brokerId>": {"<logDir>": bytes}}, or {"<brokerId>":
// bytes} for every dir of that broker; a value is a number or a string with K/M/G/T), else with --utilisation from the totalBytes of
// --log-dirs when above 0 (Kafka >= 3.3), else from --default-capacity; a usable dir of a listed broker with none is a usage
// error.  The plan keeps its format; the report gains peak_before_ppm, peak_after_ppm, lower_bound_ppm and proof per broker, the two
// peaks in ppm for the call, and a warning line for a dir whose base alone exceeds its capacity.
// Exit status: 0 = ok, 1 = error, 2 = usage.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../include/kao.h"
#include "kao_cluster.h"
#include "kao_json.h"
#include "kao_sizes.h"

namespace {

[[noreturn]] void usage(const char *msg) {
    if (msg) std::fprintf(stderr, "kao-logdirs: %s\n", msg);
    std::fprintf(stderr,
        "usage: kao-logdirs --current <reassignment.json> --log-dirs <kafka-log-dirs output> [--broker-list <id,id,...>]\n"
        "                   [--min-gain N[K|M|G|T]] [--max-rounds N] [--dry-run] --out <file> [--report] [--device D]\n"
        "                   [--plan <reassignment.json>] [--evacuate <broker>:<dir>]... [--rebalance] [--default-size N[K|M|G|T]]\n"
        "                   [--utilisation] [--capacities <caps.json>] [--default-capacity N[K|M|G|T]]\n"
        "                   [--exchange]   (the plain balance only: not with --plan, --evacuate, --rebalance or capacities)\n"
        "writes the partitions with a replica that moves to another log dir of its broker; exit status: 0 = ok, 1 = error, 2 = usage\n");
    std::exit(2);
}

// --utilisation / --capacities / --default-capacity: where a dir's capacity comes from
struct Capacities {
    bool on = false, utilisation = false, have_default = false;
    uint64_t default_cap = 0;
    std::map<int, uint64_t> of_broker;                           // {"<brokerId>": bytes}
    std::map<std::pair<int, std::string>, uint64_t> of_dir;      // {"<brokerId>": {"<logDir>": bytes}}
    std::set<int> by_dir;                                        // brokers listed with an object
};

// --capacities: a JSON file {"<brokerId>": {"<logDir>": bytes} | bytes}, a value a number or a string, each N or N with K/M/G/T
void read_capacities(const std::string &path, Capacities &c) {
    auto value = [](const JValue &v, const std::string &what) {
        uint64_t x = 0;
        if ((v.kind != JValue::Num && v.kind != JValue::Str) || !parse_bytes(v.kind == JValue::Num ? v.raw : v.str, x))
            throw std::runtime_error("capacity of " + what + ": not a byte count");
        return x;
    };
    const std::string txt = slurp(path);
    const JValue doc = JParser(txt).parse();
    if (doc.kind != JValue::Obj) throw std::runtime_error("capacities file must be a JSON object {\"<brokerId>\": {\"<logDir>\": bytes} | bytes}");
    for (auto &kv : doc.obj) {
        if (kv.first.empty() || kv.first.size() > 9 || kv.first.find_first_not_of("0123456789") != std::string::npos)
            throw std::runtime_error("capacity of broker " + kv.first + ": not a broker id");
        const int b = std::atoi(kv.first.c_str());
        if (kv.second.kind == JValue::Obj) {
            c.by_dir.insert(b);
            for (auto &dv : kv.second.obj) c.of_dir[{b, dv.first}] = value(dv.second, "log dir " + std::to_string(b) + ":" + dv.first);
        } else {
            c.of_broker[b] = value(kv.second, "broker " + std::to_string(b));
        }
    }
}

// capacity[d] of every dir of the call: the entry of --capacities, else totalBytes > 0 under --utilisation, else the default; a dir
// with none is a usage error
std::vector<uint64_t> dir_capacities(const Capacities &c, const std::vector<int> &ids, const std::vector<std::vector<const LogDir *>> &dirs) {
    std::vector<uint64_t> out;
    std::vector<std::string> missing;
    for (size_t i = 0; i < ids.size(); ++i)
        for (auto *d : dirs[i]) {
            auto dv = c.of_dir.find({ids[i], d->name});
            auto bv = c.of_broker.find(ids[i]);
            if (c.by_dir.count(ids[i]) && dv != c.of_dir.end()) out.push_back(dv->second);
            else if (!c.by_dir.count(ids[i]) && bv != c.of_broker.end()) out.push_back(bv->second);
            else if (c.utilisation && d->has_total && d->total_bytes > 0) out.push_back(d->total_bytes);
            else if (c.have_default) out.push_back(c.default_cap);
            else missing.push_back(std::to_string(ids[i]) + ":" + d->name);
        }
    if (!missing.empty()) {
        std::string msg = "no capacity for log dirs ";
        for (size_t i = 0; i < missing.size() && i < 5; ++i) msg += (i ? ", " : "") + missing[i];
        if (missing.size() > 5) msg += " and " + std::to_string(missing.size() - 5) + " more";
        usage((msg + " (give them in --capacities, read totalBytes with --utilisation or set --default-capacity)").c_str());
    }
    if (out.empty()) out.push_back(1);   // the library takes no null pointer
    return out;
}

// floor(num * 10^6 / den) in decimal; the product passes 64 bits
std::string ppm(uint64_t num, uint64_t den) {
    unsigned __int128 v = (unsigned __int128)num * 1000000u / den;
    std::string s;
    do { s.insert(s.begin(), (char)('0' + (int)(v % 10))); v /= 10; } while (v);
    return s;
}

void warn_full(const std::vector<int> &ids, const std::vector<std::vector<const LogDir *>> &dirs, const std::vector<int32_t> &dir_start,
               const std::vector<uint64_t> &base, const std::vector<uint64_t> &cap) {
    for (size_t i = 0; i < ids.size(); ++i)
        for (size_t li = 0; li < dirs[i].size(); ++li) {
            const size_t d = (size_t)dir_start[i] + li;
            if (base[d] > cap[d])
                std::fprintf(stderr, "logdirs: warning: broker=%d dir=%s base=%llu exceeds capacity=%llu\n", ids[i], dirs[i][li]->name.c_str(),
                             (unsigned long long)base[d], (unsigned long long)cap[d]);
        }
}

// what main makes of the flags
struct Options {
    std::string cur_path, dirs_path, plan_path, out_path, brokers_csv;
    std::vector<std::pair<int, std::string>> evacuate;
    bool have_list = false, rebalance = false, have_default = false, exchange = false, dry_run = false, report = false;
    uint64_t default_size = 0, min_gain = 0;
    int max_rounds = 0, device = 0;
    Capacities caps;
    bool placing() const { return !plan_path.empty() || !evacuate.empty(); }   // kao_place_logdirs, not kao_balance_logdirs
};

using Rows = std::map<Key, std::vector<int>>;

// the rows of a reassignment document by (topic, partition)
Rows rows_of(const std::string &path, const char *what) {
    Rows out;
    const std::string txt = slurp(path);
    const JValue doc = JParser(txt).parse();
    const JValue *parts = doc.get("partitions");
    for (size_t i = 0; parts && i < parts->arr.size(); ++i) {
        const JValue &e = parts->arr[i];
        const JValue *t = e.get("topic"), *p = e.get("partition"), *r = e.get("replicas");
        if (!t || !p || !r || r->kind != JValue::Arr) throw std::runtime_error("partition entry needs topic/partition/replicas");
        const Key k{t->str, (int)p->num};
        if (out.count(k)) throw std::runtime_error(std::string(what) + ": partition " + k.first + "-" + std::to_string(k.second) + " listed twice");
        std::vector<int> &reps = out[k];
        for (auto &x : r->arr) reps.push_back((int)x.num);
    }
    return out;
}

// The documents as the arrays of the call (the mapping is in the head of this file).  The balance call is the placement with no
// plan and no evacuation: every replica a resident, nothing stranded.  Moved, never copied: the pointers go into its own maps.
struct Slot { const Key *key; const std::vector<int> *row; int j; };
struct Mapping {
    std::map<int, std::vector<LogDir>> table;
    Rows by_key, plan;
    std::vector<int> ids, skipped;                           // per broker: its id, its dirs left out for their error
    std::vector<std::vector<const LogDir *>> stay, gone;     // per broker: its usable dirs byte-wise ascending, the evacuated ones apart
    std::vector<std::set<std::string>> out_of;               // per broker: the names of its evacuated dirs
    std::vector<int32_t> dir_start{0};
    std::vector<std::string> flat;                           // global dir index -> name
    std::vector<int32_t> broker, dir;                        // per replica; dir -1 = homeless
    std::vector<uint64_t> size;
    std::vector<Slot> slots;
    std::vector<uint64_t> base;
    std::vector<unsigned long long> stranded;                // per broker: bytes of the entries of its evacuated dirs that are not planned
    Mapping() = default;
    Mapping(Mapping &&) = default;
    Mapping(const Mapping &) = delete;
};

Mapping map_documents(const Options &o) {
    Mapping m;
    m.by_key = rows_of(o.cur_path, "current");
    if (!o.plan_path.empty()) m.plan = rows_of(o.plan_path, "plan");
    for (auto &kv : m.plan) {
        const std::string what = kv.first.first + "-" + std::to_string(kv.first.second);
        if (!m.by_key.count(kv.first)) throw std::runtime_error("plan: partition " + what + " is not in the current assignment");
        if (std::set<int>(kv.second.begin(), kv.second.end()).size() != kv.second.size()) throw std::runtime_error("plan: partition " + what + " lists a broker twice");
    }
    m.table = load_log_dirs(o.dirs_path);
    if (o.have_list) {
        for (auto &t : split(o.brokers_csv, ',')) if (!t.empty()) m.ids.push_back(std::atoi(t.c_str()));
    } else {
        for (auto &kv : m.table) m.ids.push_back(kv.first);
    }
    if (m.ids.empty()) throw std::runtime_error("empty broker list");
    std::map<int, int> dense;
    for (size_t i = 0; i < m.ids.size(); ++i) if (!dense.emplace(m.ids[i], (int)i).second) throw std::runtime_error("duplicate id in broker list");
    const size_t B = m.ids.size();
    m.out_of.resize(B);
    for (auto &ev : o.evacuate) {
        auto di = dense.find(ev.first);
        auto it = m.table.find(ev.first);
        bool ok = false;
        if (di != dense.end() && it != m.table.end())
            for (auto &d : it->second) ok |= d.name == ev.second && !d.failed;
        if (!ok) throw std::runtime_error("evacuate: " + std::to_string(ev.first) + ":" + ev.second + " is not a usable log dir of a listed broker");
        m.out_of[(size_t)di->second].insert(ev.second);
    }
    std::map<Key, uint64_t> psize;   // the largest non-future size of a partition anywhere: the size of an arrival
    for (auto &kv : m.table)
        for (auto &d : kv.second)
            for (auto &e : d.entries)
                if (!e.future) { uint64_t &x = psize[e.key]; x = std::max(x, e.size); }

    // the usable dirs of every broker, byte-wise ascending, without the evacuated ones; where each partition sits on it
    struct Held { int dir; uint64_t size; };
    m.stay.resize(B);
    m.gone.resize(B);
    m.skipped.assign(B, 0);
    std::vector<std::map<Key, Held>> where(B);
    std::vector<std::map<Key, uint64_t>> leaving(B);
    for (size_t i = 0; i < B; ++i) {
        std::vector<const LogDir *> usable;
        auto it = m.table.find(m.ids[i]);
        if (it != m.table.end())
            for (auto &d : it->second) {
                if (d.failed) ++m.skipped[i];
                else usable.push_back(&d);
            }
        std::sort(usable.begin(), usable.end(), [](const LogDir *x, const LogDir *y) { return x->name < y->name; });
        for (auto *d : usable) (m.out_of[i].count(d->name) ? m.gone : m.stay)[i].push_back(d);
        if (!m.out_of[i].empty() && m.stay[i].empty()) throw std::runtime_error("evacuate: broker " + std::to_string(m.ids[i]) + " is left without a usable log dir");
        for (auto *d : usable) {
            const bool out = m.out_of[i].count(d->name) != 0;
            const int li = out ? 0 : (int)(std::find(m.stay[i].begin(), m.stay[i].end(), d) - m.stay[i].begin());
            for (auto &e : d->entries) {
                if (e.future) continue;
                if (where[i].count(e.key) || leaving[i].count(e.key))
                    throw std::runtime_error("log-dirs: broker " + std::to_string(m.ids[i]) + " holds partition " + e.key.first + "-" + std::to_string(e.key.second) + " twice");
                if (out) leaving[i][e.key] = e.size;
                else where[i][e.key] = Held{m.dir_start.back() + li, e.size};
            }
        }
        for (auto *d : m.stay[i]) m.flat.push_back(d->name);
        m.dir_start.push_back(m.dir_start.back() + (int32_t)m.stay[i].size());
    }

    // the replicas: residents, and the homeless ones (dir -1) of evacuated dirs and of the plan's arrivals
    std::set<std::pair<int, Key>> claimed, rescued, departed;
    for (auto &kv : m.by_key) {
        auto pl = m.plan.find(kv.first);
        const std::vector<int> &row = pl == m.plan.end() ? kv.second : pl->second;
        const std::set<int> was(kv.second.begin(), kv.second.end());
        for (int x : was)
            if (std::find(row.begin(), row.end(), x) == row.end() && dense.count(x)) departed.insert({dense[x], kv.first});
        for (size_t j = 0; j < row.size(); ++j) {
            auto di = dense.find(row[j]);
            if (di == dense.end()) continue;
            const size_t i = (size_t)di->second;
            int32_t d = -1;
            uint64_t sz = 0;
            auto lv = leaving[i].find(kv.first);
            if (lv != leaving[i].end()) {   // its dir is being evacuated
                sz = lv->second;
                rescued.insert({di->second, kv.first});
            } else if (was.count(row[j])) {
                auto h = where[i].find(kv.first);
                if (h == where[i].end()) continue;
                d = h->second.dir;
                sz = h->second.size;
                claimed.insert({di->second, kv.first});
            } else {   // an arrival
                if (m.stay[i].empty()) continue;
                auto ps = psize.find(kv.first);
                if (ps != psize.end()) sz = ps->second;
                else if (o.have_default) sz = o.default_size;
                else
                    throw std::runtime_error("log-dirs: no size for partition " + kv.first.first + "-" + std::to_string(kv.first.second) + ", which the plan brings to broker " +
                                             std::to_string(row[j]) + " (give a default size)");
            }
            m.broker.push_back(di->second);
            m.dir.push_back(d);
            m.size.push_back(sz);
            m.slots.push_back(Slot{&kv.first, &row, (int)j});
        }
    }
    m.base.assign((size_t)std::max(m.dir_start.back(), 1), 0);
    m.stranded.assign(B, 0);
    for (size_t i = 0; i < B; ++i) {
        for (size_t li = 0; li < m.stay[i].size(); ++li)
            for (auto &e : m.stay[i][li]->entries) {
                if (!e.future && departed.count({(int)i, e.key})) continue;
                if (e.future || !claimed.count({(int)i, e.key})) m.base[(size_t)m.dir_start[i] + li] += e.size;
            }
        for (auto *d : m.gone[i])
            for (auto &e : d->entries)
                if (e.future || !rescued.count({(int)i, e.key})) m.stranded[i] += e.size;
    }
    return m;
}

// what a call gives back; a call by bytes writes the first word of a peak alone
struct Called {
    int32_t n_placed = 0, n_moved = 0, status = 0;
    uint64_t bytes_placed = 0, bytes_moved = 0, before[2] = {0, 1}, after[2] = {0, 1};
    int64_t stats[12] = {0};
    std::vector<uint64_t> per;   // [B, W]
    size_t W = 0;
};

// the entry points and the words of a broker's row in per_broker[]
enum { BALANCE, EXCHANGE, BALANCE_CAPACITY, PLACE, PLACE_CAPACITY };
struct Entry { const char *name; size_t per; };
const Entry ENTRIES[] = {{"kao_balance_logdirs", 6}, {"kao_balance_logdirs_exchange", 8}, {"kao_balance_logdirs_capacity", 10}, {"kao_place_logdirs", 8},
                         {"kao_place_logdirs_capacity", 12}};

// the one call of the library: the five entry points take their arrays in one order, the balance ones without broker[]
Called call(const Options &o, Mapping &m, const std::vector<uint64_t> &cap) {
    const int B = (int)m.ids.size(), R = (int)m.dir.size(), dry = o.dry_run ? 1 : 0;
    if (m.dir.empty()) { m.broker.push_back(0); m.dir.push_back(0); m.size.push_back(0); }   // the library takes no null pointer
    const int32_t *ds = m.dir_start.data(), *br = m.broker.data();
    const uint64_t *bs = m.base.data(), *sz = m.size.data();
    int32_t *dir = m.dir.data();
    const int entry = o.placing() ? (o.caps.on ? PLACE_CAPACITY : PLACE) : o.caps.on ? BALANCE_CAPACITY : o.exchange ? EXCHANGE : BALANCE;
    const char *const name = ENTRIES[entry].name;
    Called c;
    c.W = ENTRIES[entry].per;
    c.per.assign((size_t)B * c.W, 0);
    int rc;
    switch (entry) {
    case BALANCE:
        rc = kao_balance_logdirs(B, ds, bs, R, dir, sz, o.min_gain, o.max_rounds, dry, &c.n_moved, &c.bytes_moved, c.before, c.after, c.per.data(), &c.status, c.stats);
        break;
    case EXCHANGE:
        rc = kao_balance_logdirs_exchange(B, ds, bs, R, dir, sz, o.min_gain, o.max_rounds, dry, &c.n_moved, &c.bytes_moved, c.before, c.after, c.per.data(), &c.status,
                                          c.stats);
        break;
    case BALANCE_CAPACITY:
        rc = kao_balance_logdirs_capacity(B, ds, bs, cap.data(), R, dir, sz, o.min_gain, o.max_rounds, dry, &c.n_moved, &c.bytes_moved, c.before, c.after, c.per.data(),
                                          &c.status, c.stats);
        break;
    case PLACE:
        rc = kao_place_logdirs(B, ds, bs, R, br, dir, sz, o.rebalance ? 1 : 0, o.min_gain, o.max_rounds, dry, &c.n_placed, &c.bytes_placed, &c.n_moved, &c.bytes_moved,
                               c.before, c.after, c.per.data(), &c.status, c.stats);
        break;
    default:   // PLACE_CAPACITY
        rc = kao_place_logdirs_capacity(B, ds, bs, cap.data(), R, br, dir, sz, o.rebalance ? 1 : 0, o.min_gain, o.max_rounds, dry, &c.n_placed, &c.bytes_placed,
                                        &c.n_moved, &c.bytes_moved, c.before, c.after, c.per.data(), &c.status, c.stats);
    }
    if (rc) throw std::runtime_error(std::string(name) + ": " + kao_strerror(rc) + " " + kao_last_error());
    return c;
}

// the names of a broker's columns once the capacity words are folded away, and of stats[]
const char *const BALANCE_COLUMNS[] = {"peak_before", "peak_after", "lower_bound", "moved", "bytes_moved", "rounds"};
const char *const PLACE_COLUMNS[] = {"peak_before", "peak_after", "lower_bound", "placed", "bytes_placed", "moved", "bytes_moved", "rounds"};
const char *const STAT_KEYS[] = {"brokers_moved", "rounds", "moves", "proposals", "launches", "stopped_by_max_rounds", "proven", "max_rounds_of_a_broker",
                                 "exchange_rounds", "exchanges", "exchange_proposals", "brokers_lowered_by_exchange"};   // the last four with --exchange
const char *const PLACE_STAT_KEYS[] = {"brokers_placed", "brokers_moved", "rounds", "moves", "proposals", "launches", "stopped_by_max_rounds", "proven",
                                       "max_rounds_of_a_broker", "max_homeless_of_a_broker"};

template <class T> void field(std::string &line, const char *key, T value) { line += std::string(" ") + key + "=" + std::to_string(value); }

// --report: one line per broker and one for the call, to stderr.  dir0 is dir[] as the mapping made it.
void report(const Options &o, const Mapping &m, const std::vector<int32_t> &dir0, const std::vector<uint64_t> &cap, const Called &c) {
    const bool placing = o.placing(), by_cap = o.caps.on;
    const size_t B = m.ids.size(), n_cols = placing ? 8 : 6;
    if (by_cap) warn_full(m.ids, m.stay, m.dir_start, m.base, cap);
    std::vector<int> residents(B, 0), homeless(B, 0);
    unsigned long long total = 0, all_skipped = 0, all_out = 0, all_stranded = 0;
    int all_home = 0;
    for (size_t r = 0; r < dir0.size(); ++r) {
        ++(dir0[r] < 0 ? homeless : residents)[(size_t)m.broker[r]];
        all_home += dir0[r] < 0;
        total += m.size[r];
    }
    for (int d = 0; d < m.dir_start.back(); ++d) total += m.base[(size_t)d];
    for (size_t i = 0; i < B; ++i) {
        const uint64_t *q = c.per.data() + i * c.W;   // with capacities {peak_before, cap, peak_after, cap, bound num, den, <the other columns>, proof}
        all_skipped += (unsigned long long)m.skipped[i];
        all_out += m.out_of[i].size();
        all_stranded += m.stranded[i];
        std::string line = "logdirs: broker=" + std::to_string(m.ids[i]);
        field(line, "dirs", m.stay[i].size());
        field(line, "skipped_dirs", m.skipped[i]);
        if (placing) field(line, "evacuated_dirs", m.out_of[i].size());
        field(line, "replicas", residents[i] + homeless[i]);
        if (placing) { field(line, "residents", residents[i]); field(line, "homeless", homeless[i]); }
        for (size_t k = 0; k < n_cols; ++k) field(line, (placing ? PLACE_COLUMNS : BALANCE_COLUMNS)[k], !by_cap ? q[k] : k < 3 ? q[2 * k] : q[k + 3]);
        if (placing) field(line, "stranded_bytes", m.stranded[i]);
        if (by_cap) line += " peak_before_ppm=" + ppm(q[0], q[1]) + " peak_after_ppm=" + ppm(q[2], q[3]) + " lower_bound_ppm=" + ppm(q[4], q[5]) + " proof=" + std::to_string(q[c.W - 1]);
        if (o.exchange) { field(line, "exchange_rounds", q[6]); field(line, "exchanges", q[7]); }
        std::fprintf(stderr, "%s\n", line.c_str());
    }
    std::string line = std::string("logdirs: status=") + (c.status == KAO_STATUS_OPTIMAL_PROVEN ? "OPTIMAL_PROVEN" : "FEASIBLE_BOUND_GAP");
    field(line, "brokers", B);
    field(line, "dirs", m.dir_start.back());
    field(line, "skipped_dirs", all_skipped);
    if (placing) field(line, "evacuated_dirs", all_out);
    field(line, "replicas", dir0.size());
    if (placing) { field(line, "residents", (int)dir0.size() - all_home); field(line, "homeless", all_home); }
    field(line, "peak_before", c.before[0]);
    field(line, "peak_after", c.after[0]);
    if (placing) { field(line, "replicas_placed", c.n_placed); field(line, "bytes_placed", c.bytes_placed); }
    field(line, "replicas_moved", c.n_moved);
    field(line, "bytes_moved", c.bytes_moved);
    field(line, "bytes_total", total);
    if (placing) field(line, "stranded_bytes", all_stranded);
    for (size_t k = 0; k < (placing ? 10u : o.exchange ? 12u : 8u); ++k) field(line, (placing ? PLACE_STAT_KEYS : STAT_KEYS)[k], c.stats[k]);
    if (by_cap) line += " peak_before_ppm=" + ppm(c.before[0], c.before[1]) + " peak_after_ppm=" + ppm(c.after[0], c.after[1]);
    std::fprintf(stderr, "%s\n", line.c_str());
}

// the partitions of the plan and those with a placed or moved replica, in (topic, partition) order; none with --dry-run
void write_plan(const Options &o, const Mapping &m, const std::vector<int32_t> &dir0) {
    std::map<Key, std::vector<std::string>> lists;
    if (!o.dry_run) {
        for (auto &kv : m.plan) lists[kv.first] = std::vector<std::string>(kv.second.size(), "any");
        for (size_t r = 0; r < dir0.size(); ++r) {
            if (m.dir[r] == dir0[r]) continue;
            const Slot &sl = m.slots[r];
            auto it = lists.find(*sl.key);
            if (it == lists.end()) it = lists.emplace(*sl.key, std::vector<std::string>(sl.row->size(), "any")).first;
            it->second[(size_t)sl.j] = m.flat[(size_t)m.dir[r]];
        }
    }
    std::string body;
    int n_out = 0;
    for (auto &kv : lists) {
        auto pl = m.plan.find(kv.first);
        const std::vector<int> &row = pl == m.plan.end() ? m.by_key.at(kv.first) : pl->second;
        body += (n_out++ ? ",\n" : "\n");
        body += "    {\"topic\":" + quoted(kv.first.first) + ",\"partition\":" + std::to_string(kv.first.second) + ",\"replicas\":[";
        for (size_t k = 0; k < row.size(); ++k) body += (k ? "," : "") + std::to_string(row[k]);
        body += "],\"log_dirs\":[";
        for (size_t k = 0; k < kv.second.size(); ++k) body += (k ? "," : "") + quoted(kv.second[k]);
        body += "]}";
    }
    std::ofstream f(o.out_path);
    f << "{\"version\":1,\"partitions\":[" << body << "\n]}\n";
    f.close();
    if (!f) throw std::runtime_error("cannot write " + o.out_path);
}

// documents -> arrays -> the call -> report -> plan; every input error comes before the device is touched
void run(const Options &o) {
    Mapping m = map_documents(o);
    const std::vector<uint64_t> cap = o.caps.on ? dir_capacities(o.caps, m.ids, m.stay) : std::vector<uint64_t>();
    const std::vector<int32_t> dir0 = m.dir;
    const int rc = kao_init(o.device);
    if (rc) throw std::runtime_error(std::string("kao_init: ") + kao_strerror(rc) + " " + kao_last_error());
    const Called c = call(o, m, cap);
    if (o.report) report(o, m, dir0, cap, c);
    write_plan(o, m, dir0);
    kao_shutdown();
}

}  // namespace

int main(int argc, char **argv) {
    Options o;
    std::string caps_path;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto need = [&](const char *flag) -> std::string { if (i + 1 >= argc) usage((std::string(flag) + " needs a value").c_str()); return argv[++i]; };
        if (a == "--current") o.cur_path = need("--current");
        else if (a == "--log-dirs") o.dirs_path = need("--log-dirs");
        else if (a == "--broker-list") { o.brokers_csv = need("--broker-list"); o.have_list = true; }
        else if (a == "--out") o.out_path = need("--out");
        else if (a == "--dry-run") o.dry_run = true;
        else if (a == "--device") o.device = std::atoi(need("--device").c_str());
        else if (a == "--report") o.report = true;
        else if (a == "--plan") o.plan_path = need("--plan");
        else if (a == "--rebalance") o.rebalance = true;
        else if (a == "--exchange") o.exchange = true;
        else if (a == "--evacuate") {
            const std::string v = need("--evacuate");
            const size_t colon = v.find(':');
            const std::string b = colon == std::string::npos ? "" : v.substr(0, colon);
            const std::string digits = !b.empty() && b[0] == '-' ? b.substr(1) : b;
            if (colon == std::string::npos || colon + 1 >= v.size() || digits.empty() || b.size() > 10 || digits.find_first_not_of("0123456789") != std::string::npos)
                usage("--evacuate needs BROKER:DIR");
            o.evacuate.emplace_back(std::atoi(b.c_str()), v.substr(colon + 1));
        } else if (a == "--default-size") {
            if (!parse_bytes(need("--default-size"), o.default_size)) usage("--default-size needs a byte count (N, or N with K/M/G/T)");
            o.have_default = true;
        } else if (a == "--utilisation") {
            o.caps.utilisation = true;
        } else if (a == "--capacities") {
            caps_path = need("--capacities");
        } else if (a == "--default-capacity") {
            if (!parse_bytes(need("--default-capacity"), o.caps.default_cap)) usage("--default-capacity needs a byte count (N, or N with K/M/G/T)");
            o.caps.have_default = true;
        } else if (a == "--min-gain") {
            if (!parse_bytes(need("--min-gain"), o.min_gain)) usage("--min-gain needs a byte count (N, or N with K/M/G/T)");
        } else if (a == "--max-rounds") {
            const std::string v = need("--max-rounds");
            if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos) usage("--max-rounds needs a value >= 0");
            o.max_rounds = std::atoi(v.c_str());
        } else if (a == "-h" || a == "--help") usage(nullptr);
        else usage(("unknown flag " + a).c_str());
    }
    if (o.cur_path.empty() || o.dirs_path.empty() || o.out_path.empty()) usage("--current, --log-dirs and --out are required");
    if ((o.rebalance || o.have_default) && !o.placing()) usage("--rebalance and --default-size need --plan or --evacuate");
    o.caps.on = o.caps.utilisation || !caps_path.empty() || o.caps.have_default;
    if (o.exchange && (o.placing() || o.caps.on))
        usage("--exchange cannot be combined with --utilisation, --capacities, --default-capacity, --plan, --evacuate or --rebalance");
    if (!caps_path.empty()) {
        std::string msg;
        try {
            read_capacities(caps_path, o.caps);
        } catch (const std::exception &e) {
            msg = std::string("--capacities: ") + e.what();
        }
        if (!msg.empty()) usage(msg.c_str());
    }
    try {
        run(o);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "kao-logdirs: %s\n", e.what());
        return 1;
    }
    return 0;
}
