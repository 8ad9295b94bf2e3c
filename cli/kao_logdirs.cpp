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

// --plan / --evacuate: kao_place_logdirs (the mapping is in the head of this file).  Returns when the plan is written.
void place(const Capacities &caps, const std::string &cur_path, const std::string &dirs_path, const std::string &plan_path, const std::vector<std::pair<int, std::string>> &evacuate,
           bool have_list, const std::string &brokers_csv, bool rebalance, bool have_default, uint64_t default_size, uint64_t min_gain, int max_rounds,
           bool dry_run, bool report, int device, const std::string &out_path) {
    auto rows_of = [](const std::string &path, const char *what) {
        std::map<Key, std::vector<int>> out;
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
    };
    const std::map<Key, std::vector<int>> by_key = rows_of(cur_path, "current");
    std::map<Key, std::vector<int>> plan;
    if (!plan_path.empty()) plan = rows_of(plan_path, "plan");
    for (auto &kv : plan) {
        const std::string what = kv.first.first + "-" + std::to_string(kv.first.second);
        if (!by_key.count(kv.first)) throw std::runtime_error("plan: partition " + what + " is not in the current assignment");
        if (std::set<int>(kv.second.begin(), kv.second.end()).size() != kv.second.size()) throw std::runtime_error("plan: partition " + what + " lists a broker twice");
    }
    const std::map<int, std::vector<LogDir>> table = load_log_dirs(dirs_path);
    std::vector<int> ids;
    if (have_list) {
        for (auto &t : split(brokers_csv, ',')) if (!t.empty()) ids.push_back(std::atoi(t.c_str()));
    } else {
        for (auto &kv : table) ids.push_back(kv.first);
    }
    if (ids.empty()) throw std::runtime_error("empty broker list");
    std::map<int, int> dense;
    for (size_t i = 0; i < ids.size(); ++i) if (!dense.emplace(ids[i], (int)i).second) throw std::runtime_error("duplicate id in broker list");
    const int B = (int)ids.size();
    std::vector<std::set<std::string>> out_of((size_t)B);
    for (auto &ev : evacuate) {
        auto di = dense.find(ev.first);
        auto it = table.find(ev.first);
        bool ok = false;
        if (di != dense.end() && it != table.end())
            for (auto &d : it->second) ok |= d.name == ev.second && !d.failed;
        if (!ok) throw std::runtime_error("evacuate: " + std::to_string(ev.first) + ":" + ev.second + " is not a usable log dir of a listed broker");
        out_of[(size_t)di->second].insert(ev.second);
    }
    std::map<Key, uint64_t> psize;   // the largest non-future size of a partition anywhere: the size of an arrival
    for (auto &kv : table)
        for (auto &d : kv.second)
            for (auto &e : d.entries)
                if (!e.future) { uint64_t &x = psize[e.key]; x = std::max(x, e.size); }

    // the usable dirs of every broker, byte-wise ascending, without the evacuated ones; where each partition sits on it
    struct Held { int dir; uint64_t size; };
    std::vector<std::vector<const LogDir *>> stay((size_t)B), gone((size_t)B);
    std::vector<int> skipped((size_t)B, 0);
    std::vector<int32_t> dir_start(1, 0);
    std::vector<std::map<Key, Held>> where((size_t)B);
    std::vector<std::map<Key, uint64_t>> leaving((size_t)B);
    std::vector<std::string> flat;   // global dir index -> name
    for (int i = 0; i < B; ++i) {
        std::vector<const LogDir *> usable;
        auto it = table.find(ids[(size_t)i]);
        if (it != table.end())
            for (auto &d : it->second) {
                if (d.failed) ++skipped[(size_t)i];
                else usable.push_back(&d);
            }
        std::sort(usable.begin(), usable.end(), [](const LogDir *x, const LogDir *y) { return x->name < y->name; });
        for (auto *d : usable) (out_of[(size_t)i].count(d->name) ? gone : stay)[(size_t)i].push_back(d);
        if (!out_of[(size_t)i].empty() && stay[(size_t)i].empty())
            throw std::runtime_error("evacuate: broker " + std::to_string(ids[(size_t)i]) + " is left without a usable log dir");
        for (auto *d : usable) {
            const bool out = out_of[(size_t)i].count(d->name) != 0;
            const int li = out ? 0 : (int)(std::find(stay[(size_t)i].begin(), stay[(size_t)i].end(), d) - stay[(size_t)i].begin());
            for (auto &e : d->entries) {
                if (e.future) continue;
                if (where[(size_t)i].count(e.key) || leaving[(size_t)i].count(e.key))
                    throw std::runtime_error("log-dirs: broker " + std::to_string(ids[(size_t)i]) + " holds partition " + e.key.first + "-" + std::to_string(e.key.second) + " twice");
                if (out) leaving[(size_t)i][e.key] = e.size;
                else where[(size_t)i][e.key] = Held{dir_start.back() + li, e.size};
            }
        }
        for (auto *d : stay[(size_t)i]) flat.push_back(d->name);
        dir_start.push_back(dir_start.back() + (int32_t)stay[(size_t)i].size());
    }
    const int D = dir_start.back();

    // the replicas: residents, and the homeless ones (dir -1) of evacuated dirs and of the plan's arrivals
    struct Slot { const Key *key; const std::vector<int> *row; int j; };
    std::vector<int32_t> broker, dir;
    std::vector<uint64_t> size;
    std::vector<Slot> slots;
    std::set<std::pair<int, Key>> claimed, rescued, departed;
    for (auto &kv : by_key) {
        auto pl = plan.find(kv.first);
        const std::vector<int> &row = pl == plan.end() ? kv.second : pl->second;
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
                if (stay[i].empty()) continue;
                auto ps = psize.find(kv.first);
                if (ps != psize.end()) sz = ps->second;
                else if (have_default) sz = default_size;
                else
                    throw std::runtime_error("log-dirs: no size for partition " + kv.first.first + "-" + std::to_string(kv.first.second) + ", which the plan brings to broker " +
                                             std::to_string(row[j]) + " (give a default size)");
            }
            broker.push_back(di->second);
            dir.push_back(d);
            size.push_back(sz);
            slots.push_back(Slot{&kv.first, &row, (int)j});
        }
    }
    std::vector<uint64_t> base((size_t)std::max(D, 1), 0);
    std::vector<unsigned long long> stranded((size_t)B, 0);
    for (int i = 0; i < B; ++i) {
        for (size_t li = 0; li < stay[(size_t)i].size(); ++li)
            for (auto &e : stay[(size_t)i][li]->entries) {
                if (!e.future && departed.count({i, e.key})) continue;
                if (e.future || !claimed.count({i, e.key})) base[(size_t)dir_start[(size_t)i] + li] += e.size;
            }
        for (auto *d : gone[(size_t)i])
            for (auto &e : d->entries)
                if (e.future || !rescued.count({i, e.key})) stranded[(size_t)i] += e.size;
    }
    const int R = (int)dir.size();
    const std::vector<int32_t> dir0 = dir;
    if (dir.empty()) { broker.push_back(0); dir.push_back(0); size.push_back(0); }   // the library takes no null pointer
    const std::vector<uint64_t> cap = caps.on ? dir_capacities(caps, ids, stay) : std::vector<uint64_t>();

    int rc = kao_init(device);
    if (rc) throw std::runtime_error(std::string("kao_init: ") + kao_strerror(rc) + " " + kao_last_error());
    int32_t n_placed = 0, n_moved = 0, status = 0;
    uint64_t bytes_placed = 0, bytes_moved = 0, before[2] = {0, 1}, after[2] = {0, 1};
    int64_t stats[10] = {0};
    const size_t W = caps.on ? 12 : 8;
    std::vector<uint64_t> per((size_t)B * W, 0);
    if (caps.on) {
        rc = kao_place_logdirs_capacity(B, dir_start.data(), base.data(), cap.data(), R, broker.data(), dir.data(), size.data(), rebalance ? 1 : 0, min_gain,
                                        max_rounds, dry_run ? 1 : 0, &n_placed, &bytes_placed, &n_moved, &bytes_moved, before, after, per.data(), &status, stats);
        if (rc) throw std::runtime_error(std::string("kao_place_logdirs_capacity: ") + kao_strerror(rc) + " " + kao_last_error());
    } else {
        rc = kao_place_logdirs(B, dir_start.data(), base.data(), R, broker.data(), dir.data(), size.data(), rebalance ? 1 : 0, min_gain, max_rounds, dry_run ? 1 : 0,
                               &n_placed, &bytes_placed, &n_moved, &bytes_moved, before, after, per.data(), &status, stats);
        if (rc) throw std::runtime_error(std::string("kao_place_logdirs: ") + kao_strerror(rc) + " " + kao_last_error());
    }
    if (report) {
        if (caps.on) warn_full(ids, stay, dir_start, base, cap);
        std::vector<int> residents((size_t)B, 0), homeless((size_t)B, 0);
        unsigned long long total = 0, all_skipped = 0, all_out = 0, all_stranded = 0;
        int all_res = 0, all_home = 0;
        for (int r = 0; r < R; ++r) {
            ++(dir0[(size_t)r] < 0 ? homeless : residents)[(size_t)broker[(size_t)r]];
            ++(dir0[(size_t)r] < 0 ? all_home : all_res);
            total += size[(size_t)r];
        }
        for (int d = 0; d < D; ++d) total += base[(size_t)d];
        for (int i = 0; i < B; ++i) {
            const uint64_t *q = per.data() + (size_t)i * W;
            // with capacities {peak_before, cap, peak_after, cap, bound num, den, placed, bytes_placed, moved, bytes_moved, rounds, proof}
            const uint64_t p[8] = {q[0], caps.on ? q[2] : q[1], caps.on ? q[4] : q[2], caps.on ? q[6] : q[3], caps.on ? q[7] : q[4], caps.on ? q[8] : q[5],
                                   caps.on ? q[9] : q[6], caps.on ? q[10] : q[7]};
            all_skipped += (unsigned long long)skipped[(size_t)i];
            all_out += (unsigned long long)out_of[(size_t)i].size();
            all_stranded += stranded[(size_t)i];
            std::fprintf(stderr, "logdirs: broker=%d dirs=%d skipped_dirs=%d evacuated_dirs=%d replicas=%d residents=%d homeless=%d peak_before=%llu peak_after=%llu "
                                 "lower_bound=%llu placed=%llu bytes_placed=%llu moved=%llu bytes_moved=%llu rounds=%llu stranded_bytes=%llu",
                         ids[(size_t)i], (int)stay[(size_t)i].size(), skipped[(size_t)i], (int)out_of[(size_t)i].size(), residents[(size_t)i] + homeless[(size_t)i],
                         residents[(size_t)i], homeless[(size_t)i], (unsigned long long)p[0], (unsigned long long)p[1], (unsigned long long)p[2], (unsigned long long)p[3],
                         (unsigned long long)p[4], (unsigned long long)p[5], (unsigned long long)p[6], (unsigned long long)p[7], stranded[(size_t)i]);
            if (caps.on)
                std::fprintf(stderr, " peak_before_ppm=%s peak_after_ppm=%s lower_bound_ppm=%s proof=%llu", ppm(q[0], q[1]).c_str(), ppm(q[2], q[3]).c_str(),
                             ppm(q[4], q[5]).c_str(), (unsigned long long)q[11]);
            std::fprintf(stderr, "\n");
        }
        std::fprintf(stderr, "logdirs: status=%s brokers=%d dirs=%d skipped_dirs=%llu evacuated_dirs=%llu replicas=%d residents=%d homeless=%d peak_before=%llu "
                             "peak_after=%llu replicas_placed=%d bytes_placed=%llu replicas_moved=%d bytes_moved=%llu bytes_total=%llu stranded_bytes=%llu "
                             "brokers_placed=%lld brokers_moved=%lld rounds=%lld moves=%lld proposals=%lld launches=%lld stopped_by_max_rounds=%lld proven=%lld "
                             "max_rounds_of_a_broker=%lld max_homeless_of_a_broker=%lld",
                     status == KAO_STATUS_OPTIMAL_PROVEN ? "OPTIMAL_PROVEN" : "FEASIBLE_BOUND_GAP", B, D, all_skipped, all_out, R, all_res, all_home,
                     (unsigned long long)before[0], (unsigned long long)after[0], n_placed, (unsigned long long)bytes_placed, n_moved, (unsigned long long)bytes_moved, total,
                     all_stranded, (long long)stats[0], (long long)stats[1], (long long)stats[2], (long long)stats[3], (long long)stats[4], (long long)stats[5],
                     (long long)stats[6], (long long)stats[7], (long long)stats[8], (long long)stats[9]);
        if (caps.on) std::fprintf(stderr, " peak_before_ppm=%s peak_after_ppm=%s", ppm(before[0], before[1]).c_str(), ppm(after[0], after[1]).c_str());
        std::fprintf(stderr, "\n");
    }
    // the partitions of the plan and those with a placed or moved replica, in (topic, partition) order
    std::map<Key, std::vector<std::string>> lists;
    if (!dry_run) {
        for (auto &kv : plan) lists[kv.first] = std::vector<std::string>(kv.second.size(), "any");
        for (int r = 0; r < R; ++r) {
            if (dir[(size_t)r] == dir0[(size_t)r]) continue;
            const Slot &sl = slots[(size_t)r];
            auto it = lists.find(*sl.key);
            if (it == lists.end()) it = lists.emplace(*sl.key, std::vector<std::string>(sl.row->size(), "any")).first;
            it->second[(size_t)sl.j] = flat[(size_t)dir[(size_t)r]];
        }
    }
    std::string body;
    int n_out = 0;
    for (auto &kv : lists) {
        auto pl = plan.find(kv.first);
        const std::vector<int> &row = pl == plan.end() ? by_key.at(kv.first) : pl->second;
        body += (n_out++ ? ",\n" : "\n");
        body += "    {\"topic\":" + quoted(kv.first.first) + ",\"partition\":" + std::to_string(kv.first.second) + ",\"replicas\":[";
        for (size_t k = 0; k < row.size(); ++k) body += (k ? "," : "") + std::to_string(row[k]);
        body += "],\"log_dirs\":[";
        for (size_t k = 0; k < kv.second.size(); ++k) body += (k ? "," : "") + quoted(kv.second[k]);
        body += "]}";
    }
    std::ofstream f(out_path);
    f << "{\"version\":1,\"partitions\":[" << body << "\n]}\n";
    f.close();
    if (!f) throw std::runtime_error("cannot write " + out_path);
    kao_shutdown();
}

}  // namespace

int main(int argc, char **argv) {
    std::string cur_path, brokers_csv, out_path, dirs_path, plan_path;
    std::vector<std::pair<int, std::string>> evacuate;
    int device = 0, max_rounds = 0;
    bool report = false, dry_run = false, have_list = false, rebalance = false, have_default = false, exchange = false;
    uint64_t min_gain = 0, default_size = 0;
    Capacities caps;
    std::string caps_path;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto need = [&](const char *flag) -> std::string { if (i + 1 >= argc) usage((std::string(flag) + " needs a value").c_str()); return argv[++i]; };
        if (a == "--current") cur_path = need("--current");
        else if (a == "--log-dirs") dirs_path = need("--log-dirs");
        else if (a == "--broker-list") { brokers_csv = need("--broker-list"); have_list = true; }
        else if (a == "--out") out_path = need("--out");
        else if (a == "--dry-run") dry_run = true;
        else if (a == "--device") device = std::atoi(need("--device").c_str());
        else if (a == "--report") report = true;
        else if (a == "--plan") plan_path = need("--plan");
        else if (a == "--rebalance") rebalance = true;
        else if (a == "--exchange") exchange = true;
        else if (a == "--evacuate") {
            const std::string v = need("--evacuate");
            const size_t colon = v.find(':');
            const std::string b = colon == std::string::npos ? "" : v.substr(0, colon);
            const std::string digits = !b.empty() && b[0] == '-' ? b.substr(1) : b;
            if (colon == std::string::npos || colon + 1 >= v.size() || digits.empty() || b.size() > 10 || digits.find_first_not_of("0123456789") != std::string::npos)
                usage("--evacuate needs BROKER:DIR");
            evacuate.emplace_back(std::atoi(b.c_str()), v.substr(colon + 1));
        } else if (a == "--default-size") {
            if (!parse_bytes(need("--default-size"), default_size)) usage("--default-size needs a byte count (N, or N with K/M/G/T)");
            have_default = true;
        } else if (a == "--utilisation") {
            caps.utilisation = true;
        } else if (a == "--capacities") {
            caps_path = need("--capacities");
        } else if (a == "--default-capacity") {
            if (!parse_bytes(need("--default-capacity"), caps.default_cap)) usage("--default-capacity needs a byte count (N, or N with K/M/G/T)");
            caps.have_default = true;
        } else if (a == "--min-gain") {
            if (!parse_bytes(need("--min-gain"), min_gain)) usage("--min-gain needs a byte count (N, or N with K/M/G/T)");
        } else if (a == "--max-rounds") {
            const std::string v = need("--max-rounds");
            if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos) usage("--max-rounds needs a value >= 0");
            max_rounds = std::atoi(v.c_str());
        } else if (a == "-h" || a == "--help") usage(nullptr);
        else usage(("unknown flag " + a).c_str());
    }
    if (cur_path.empty() || dirs_path.empty() || out_path.empty()) usage("--current, --log-dirs and --out are required");
    const bool placing = !plan_path.empty() || !evacuate.empty();
    if ((rebalance || have_default) && !placing) usage("--rebalance and --default-size need --plan or --evacuate");
    caps.on = caps.utilisation || !caps_path.empty() || caps.have_default;
    if (exchange && (placing || caps.on))
        usage("--exchange cannot be combined with --utilisation, --capacities, --default-capacity, --plan, --evacuate or --rebalance");
    if (!caps_path.empty()) {
        std::string msg;
        try {
            read_capacities(caps_path, caps);
        } catch (const std::exception &e) {
            msg = std::string("--capacities: ") + e.what();
        }
        if (!msg.empty()) usage(msg.c_str());
    }
    try {
        if (placing) {
            place(caps, cur_path, dirs_path, plan_path, evacuate, have_list, brokers_csv, rebalance, have_default, default_size, min_gain, max_rounds, dry_run, report, device,
                  out_path);
            return 0;
        }
        // the rows of --current by (topic, partition)
        std::map<Key, std::vector<int>> by_key;
        {
            const std::string txt = slurp(cur_path);
            const JValue doc = JParser(txt).parse();
            const JValue *parts = doc.get("partitions");
            for (size_t i = 0; parts && i < parts->arr.size(); ++i) {
                const JValue &e = parts->arr[i];
                const JValue *t = e.get("topic"), *p = e.get("partition"), *r = e.get("replicas");
                if (!t || !p || !r || r->kind != JValue::Arr) throw std::runtime_error("partition entry needs topic/partition/replicas");
                const Key k{t->str, (int)p->num};
                if (by_key.count(k)) throw std::runtime_error("current: partition " + k.first + "-" + std::to_string(k.second) + " listed twice");
                std::vector<int> &reps = by_key[k];
                for (auto &x : r->arr) reps.push_back((int)x.num);
            }
        }
        const std::map<int, std::vector<LogDir>> table = load_log_dirs(dirs_path);
        std::vector<int> ids;
        if (have_list) {
            for (auto &t : split(brokers_csv, ',')) if (!t.empty()) ids.push_back(std::atoi(t.c_str()));
        } else {
            for (auto &kv : table) ids.push_back(kv.first);
        }
        if (ids.empty()) throw std::runtime_error("empty broker list");
        std::map<int, int> dense;
        for (size_t i = 0; i < ids.size(); ++i) if (!dense.emplace(ids[i], (int)i).second) throw std::runtime_error("duplicate id in broker list");
        const int B = (int)ids.size();

        // the usable dirs of every broker, byte-wise ascending; where each partition sits on it
        struct Held { int dir; uint64_t size; };
        std::vector<std::vector<const LogDir *>> usable((size_t)B);
        std::vector<int> skipped((size_t)B, 0);
        std::vector<int32_t> dir_start(1, 0);
        std::vector<std::map<Key, Held>> where((size_t)B);
        std::vector<std::string> flat;   // global dir index -> name
        for (int i = 0; i < B; ++i) {
            auto it = table.find(ids[(size_t)i]);
            if (it != table.end())
                for (auto &d : it->second) {
                    if (d.failed) ++skipped[(size_t)i];
                    else usable[(size_t)i].push_back(&d);
                }
            std::sort(usable[(size_t)i].begin(), usable[(size_t)i].end(), [](const LogDir *x, const LogDir *y) { return x->name < y->name; });
            for (size_t li = 0; li < usable[(size_t)i].size(); ++li) {
                flat.push_back(usable[(size_t)i][li]->name);
                for (auto &e : usable[(size_t)i][li]->entries) {
                    if (e.future) continue;
                    if (!where[(size_t)i].emplace(e.key, Held{dir_start.back() + (int)li, e.size}).second)
                        throw std::runtime_error("log-dirs: broker " + std::to_string(ids[(size_t)i]) + " holds partition " + e.key.first + "-" + std::to_string(e.key.second) + " twice");
                }
            }
            dir_start.push_back(dir_start.back() + (int32_t)usable[(size_t)i].size());
        }
        const int D = dir_start.back();

        // the movable replicas; every other entry of a usable dir is base
        struct Slot { const Key *key; const std::vector<int> *row; int j; };
        std::vector<int32_t> dir;
        std::vector<uint64_t> size;
        std::vector<Slot> slots;
        std::set<std::pair<int, Key>> claimed;
        for (auto &kv : by_key)
            for (size_t j = 0; j < kv.second.size(); ++j) {
                auto di = dense.find(kv.second[j]);
                if (di == dense.end()) continue;
                auto h = where[(size_t)di->second].find(kv.first);
                if (h == where[(size_t)di->second].end()) continue;
                dir.push_back(h->second.dir);
                size.push_back(h->second.size);
                slots.push_back(Slot{&kv.first, &kv.second, (int)j});
                claimed.insert({di->second, kv.first});
            }
        std::vector<uint64_t> base((size_t)std::max(D, 1), 0);
        for (int i = 0; i < B; ++i)
            for (size_t li = 0; li < usable[(size_t)i].size(); ++li)
                for (auto &e : usable[(size_t)i][li]->entries)
                    if (e.future || !claimed.count({i, e.key})) base[(size_t)dir_start[(size_t)i] + li] += e.size;
        const int R = (int)dir.size();
        const std::vector<int32_t> dir0 = dir;
        if (dir.empty()) { dir.push_back(0); size.push_back(0); }   // the library takes no null pointer
        const std::vector<uint64_t> cap = caps.on ? dir_capacities(caps, ids, usable) : std::vector<uint64_t>();

        int rc = kao_init(device);
        if (rc) throw std::runtime_error(std::string("kao_init: ") + kao_strerror(rc) + " " + kao_last_error());
        int32_t n_moved = 0, status = 0;
        uint64_t bytes_moved = 0, before[2] = {0, 1}, after[2] = {0, 1};
        int64_t stats[12] = {0};
        const size_t W = caps.on ? 10 : exchange ? 8 : 6;
        std::vector<uint64_t> per((size_t)B * W, 0);
        if (exchange) {
            rc = kao_balance_logdirs_exchange(B, dir_start.data(), base.data(), R, dir.data(), size.data(), min_gain, max_rounds, dry_run ? 1 : 0, &n_moved,
                                              &bytes_moved, before, after, per.data(), &status, stats);
            if (rc) throw std::runtime_error(std::string("kao_balance_logdirs_exchange: ") + kao_strerror(rc) + " " + kao_last_error());
        } else if (caps.on) {
            rc = kao_balance_logdirs_capacity(B, dir_start.data(), base.data(), cap.data(), R, dir.data(), size.data(), min_gain, max_rounds, dry_run ? 1 : 0, &n_moved,
                                              &bytes_moved, before, after, per.data(), &status, stats);
            if (rc) throw std::runtime_error(std::string("kao_balance_logdirs_capacity: ") + kao_strerror(rc) + " " + kao_last_error());
        } else {
            rc = kao_balance_logdirs(B, dir_start.data(), base.data(), R, dir.data(), size.data(), min_gain, max_rounds, dry_run ? 1 : 0, &n_moved, &bytes_moved,
                                     before, after, per.data(), &status, stats);
            if (rc) throw std::runtime_error(std::string("kao_balance_logdirs: ") + kao_strerror(rc) + " " + kao_last_error());
        }
        if (report) {
            if (caps.on) warn_full(ids, usable, dir_start, base, cap);
            std::vector<int> replicas((size_t)B, 0);
            for (int r = 0; r < R; ++r) ++replicas[(size_t)(std::upper_bound(dir_start.begin(), dir_start.end(), dir0[(size_t)r]) - dir_start.begin() - 1)];
            unsigned long long total = 0, all_skipped = 0;
            for (int r = 0; r < R; ++r) total += size[(size_t)r];
            for (int d = 0; d < D; ++d) total += base[(size_t)d];
            for (int i = 0; i < B; ++i) {
                const uint64_t *q = per.data() + (size_t)i * W;
                // with capacities {peak_before, cap, peak_after, cap, bound num, den, moved, bytes_moved, rounds, proof}
                const uint64_t p[6] = {q[0], caps.on ? q[2] : q[1], caps.on ? q[4] : q[2], caps.on ? q[6] : q[3], caps.on ? q[7] : q[4], caps.on ? q[8] : q[5]};
                all_skipped += (unsigned long long)skipped[(size_t)i];
                std::fprintf(stderr, "logdirs: broker=%d dirs=%d skipped_dirs=%d replicas=%d peak_before=%llu peak_after=%llu lower_bound=%llu moved=%llu "
                                     "bytes_moved=%llu rounds=%llu",
                             ids[(size_t)i], (int)usable[(size_t)i].size(), skipped[(size_t)i], replicas[(size_t)i], (unsigned long long)p[0], (unsigned long long)p[1],
                             (unsigned long long)p[2], (unsigned long long)p[3], (unsigned long long)p[4], (unsigned long long)p[5]);
                if (caps.on)
                    std::fprintf(stderr, " peak_before_ppm=%s peak_after_ppm=%s lower_bound_ppm=%s proof=%llu", ppm(q[0], q[1]).c_str(), ppm(q[2], q[3]).c_str(),
                                 ppm(q[4], q[5]).c_str(), (unsigned long long)q[9]);
                if (exchange) std::fprintf(stderr, " exchange_rounds=%llu exchanges=%llu", (unsigned long long)q[6], (unsigned long long)q[7]);
                std::fprintf(stderr, "\n");
            }
            std::fprintf(stderr, "logdirs: status=%s brokers=%d dirs=%d skipped_dirs=%llu replicas=%d peak_before=%llu peak_after=%llu replicas_moved=%d "
                                 "bytes_moved=%llu bytes_total=%llu brokers_moved=%lld rounds=%lld moves=%lld proposals=%lld launches=%lld "
                                 "stopped_by_max_rounds=%lld proven=%lld max_rounds_of_a_broker=%lld",
                         status == KAO_STATUS_OPTIMAL_PROVEN ? "OPTIMAL_PROVEN" : "FEASIBLE_BOUND_GAP", B, D, all_skipped, R, (unsigned long long)before[0],
                         (unsigned long long)after[0], n_moved, (unsigned long long)bytes_moved, total, (long long)stats[0], (long long)stats[1], (long long)stats[2],
                         (long long)stats[3], (long long)stats[4], (long long)stats[5], (long long)stats[6], (long long)stats[7]);
            if (exchange)
                std::fprintf(stderr, " exchange_rounds=%lld exchanges=%lld exchange_proposals=%lld brokers_lowered_by_exchange=%lld", (long long)stats[8],
                             (long long)stats[9], (long long)stats[10], (long long)stats[11]);
            if (caps.on) std::fprintf(stderr, " peak_before_ppm=%s peak_after_ppm=%s", ppm(before[0], before[1]).c_str(), ppm(after[0], after[1]).c_str());
            std::fprintf(stderr, "\n");
        }
        // the partitions with a moved replica, in (topic, partition) order: the replicas come out in that order already
        std::string body;
        int n_out = 0;
        for (int r = 0; r < R;) {
            int e = r;
            bool moved = false;
            while (e < R && slots[(size_t)e].key == slots[(size_t)r].key) { moved |= dir[(size_t)e] != dir0[(size_t)e]; ++e; }
            if (moved) {
                const std::vector<int> &row = *slots[(size_t)r].row;
                std::vector<std::string> names(row.size(), "any");
                for (int q = r; q < e; ++q)
                    if (dir[(size_t)q] != dir0[(size_t)q]) names[(size_t)slots[(size_t)q].j] = flat[(size_t)dir[(size_t)q]];
                body += (n_out++ ? ",\n" : "\n");
                body += "    {\"topic\":" + quoted(slots[(size_t)r].key->first) + ",\"partition\":" + std::to_string(slots[(size_t)r].key->second) + ",\"replicas\":[";
                for (size_t k = 0; k < row.size(); ++k) body += (k ? "," : "") + std::to_string(row[k]);
                body += "],\"log_dirs\":[";
                for (size_t k = 0; k < names.size(); ++k) body += (k ? "," : "") + quoted(names[k]);
                body += "]}";
            }
            r = e;
        }
        std::ofstream f(out_path);
        f << "{\"version\":1,\"partitions\":[" << body << "\n]}\n";
        f.close();
        if (!f) throw std::runtime_error("cannot write " + out_path);
        kao_shutdown();
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "kao-logdirs: %s\n", e.what());
        return 1;
    }
}
