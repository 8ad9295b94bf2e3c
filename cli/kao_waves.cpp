// kao-waves -- split a reassignment plan into waves with at most K partition movements per broker per wave (kao_plan_waves,
// DESIGN.md section 4g).  The pipeline is
//
//   kao-cli --current current.json ... --out plan.json
//   kao-waves --current current.json --plan plan.json --max-per-broker K --out-prefix wave [--seed S] [--device D] [--report]
//
// With --sizes FILE (the output of `kafka-log-dirs --describe`, or {"partitions":[{"topic":..,"partition":..,"size":..}]}) and
// --max-bytes-per-broker N (bytes; K/M/G/T suffixes are powers of 1024), each wave also moves at most N bytes per broker
// (kao_plan_waves_sized): an added broker receives size[p], the source sends size[p] once per added broker.  --max-per-broker
// is then optional (0 = no count cap); --default-size N sizes the moving partitions --sizes does not list.
//
// With --headroom (needs --sizes; implied by --capacities FILE|id:bytes,.., --default-capacity N and --max-utilisation PCT) no wave
// fills a broker beyond capacity * PCT / 100, counting what it holds plus everything arriving in the wave (kao_plan_waves_headroom,
// DESIGN.md section 4v); both caps are then optional.  A broker's capacity is its --capacities entry, else the sum of its log dirs'
// totalBytes when --sizes is kafka-log-dirs output that reports one for every dir (Kafka >= 3.3), else --default-capacity.  What a
// broker holds now is the sizes of its current replicas, or all its entries of the kafka-log-dirs output when that is more.
// Partitions that fit no wave go to PREFIX-stuck.json; the tool then says "stuck: N partitions, X bytes" and exits with status 3.
//
// which writes wave1.json .. waveN.json, each a reassignment document `kafka-reassign-partitions --execute` takes on its own; run
// them in order, each after the previous one has finished.  A partition of current.json that plan.json leaves out is unchanged;
// a partition of plan.json that current.json does not list is an error.  All computation happens in libkao.so on the GPU.
// Exit status: 0 = waves written, 1 = error, 2 = usage, 3 = waves written but some partitions are stuck (--headroom).
#include <algorithm>
#include <cerrno>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../include/kao.h"
#include "kao_json.h"
#include "kao_sizes.h"

namespace {

[[noreturn]] void usage(const char *msg) {
    if (msg) std::fprintf(stderr, "kao-waves: %s\n", msg);
    std::fprintf(stderr,
        "usage: kao-waves --current <reassignment.json> --plan <reassignment.json> --max-per-broker K --out-prefix PREFIX\n"
        "                 [--seed S] [--device D] [--report]\n"
        "       sized: --sizes <kafka-log-dirs output | sizes.json> --max-bytes-per-broker N[K|M|G|T] [--default-size N]\n"
        "              (--max-per-broker optional; 0 = no count cap)\n"
        "       headroom: --headroom --sizes FILE [--capacities <caps.json | id:bytes,...>] [--default-capacity N[K|M|G|T]]\n"
        "              [--max-utilisation PCT] (each of the three implies --headroom; both caps optional; stuck partitions go to\n"
        "              PREFIX-stuck.json)\n"
        "writes PREFIX1.json .. PREFIXn.json; exit status: 0 = ok, 1 = error, 2 = usage, 3 = stuck partitions\n");
    std::exit(2);
}

// (topic, partition) -> replicas, in document order
std::vector<std::pair<Key, std::vector<int>>> entries(const std::string &path, const char *what) {
    std::string txt = slurp(path);
    JValue doc = JParser(txt).parse();
    const JValue *parts = doc.get("partitions");
    if (!parts || parts->kind != JValue::Arr) throw std::runtime_error(std::string(what) + ": missing \"partitions\" array");
    std::vector<std::pair<Key, std::vector<int>>> out;
    std::set<Key> seen;
    for (auto &e : parts->arr) {
        const JValue *t = e.get("topic"), *p = e.get("partition"), *r = e.get("replicas");
        if (!t || !p || !r || r->kind != JValue::Arr) throw std::runtime_error(std::string(what) + ": partition entry needs topic/partition/replicas");
        Key k{t->str, (int)p->num};
        if (!seen.insert(k).second) throw std::runtime_error(std::string(what) + ": partition " + k.first + "-" + std::to_string(k.second) + " listed twice");
        std::vector<int> reps;
        for (auto &x : r->arr) reps.push_back((int)x.num);
        out.emplace_back(k, std::move(reps));
    }
    return out;
}

std::string quoted(const std::string &s) {
    std::string o = "\"";
    for (char c : s) {
        if (c == '"' || c == '\\') o += '\\';
        o += c;
    }
    return o + "\"";
}

// "a, b, c, d, e and N more": the first five of a list that may be long
std::string name_list(const std::vector<std::string> &items) {
    std::string out;
    for (size_t i = 0; i < items.size() && i < 5; ++i) out += (i ? ", " : "") + items[i];
    if (items.size() > 5) out += " and " + std::to_string(items.size() - 5) + " more";
    return out;
}

// what main makes of the flags
struct Options {
    std::string cur_path, plan_path, prefix, sizes_path, caps_arg;
    int k = 0, device = 0, max_util = 100;
    unsigned long long seed = 1;
    bool report = false, have_k = false, sized = false, have_default = false, headroom = false, have_default_cap = false;
    uint64_t cap_bytes = 0, default_size = 0, default_cap = 0;
};

// The two documents as dense rows over the union broker index: every id of either document, ascending.
struct Rows {
    std::vector<Key> keys;                     // the partitions of --current, in document order
    std::vector<std::vector<int>> replicas;    // per partition: broker ids as the plan lists them, else the current ones (unchanged)
    std::vector<int> broker_id;                // dense index -> broker id
    size_t P = 0, W = 1;
    std::vector<uint16_t> c, t;                // [P, W] current and target, KAO_NONE-padded
};

Rows map_documents(const Options &o) {
    Rows r;
    const auto cur = entries(o.cur_path, "current");
    const auto plan = entries(o.plan_path, "plan");
    std::map<Key, size_t> index;
    for (auto &e : cur) {
        index[e.first] = r.keys.size();
        r.keys.push_back(e.first);
        r.replicas.push_back(e.second);
    }
    for (auto &e : plan) {
        auto it = index.find(e.first);
        if (it == index.end())
            throw std::runtime_error("plan names partition " + e.first.first + "-" + std::to_string(e.first.second) + ", which the current assignment does not have");
        r.replicas[it->second] = e.second;
    }
    r.P = cur.size();
    std::map<int, int> dense;
    for (size_t i = 0; i < r.P; ++i) {
        for (int b : cur[i].second) dense[b] = 0;
        for (int b : r.replicas[i]) dense[b] = 0;
        r.W = std::max({r.W, cur[i].second.size(), r.replicas[i].size()});
    }
    if (r.W > KAO_MAX_RF) throw std::runtime_error("more than " + std::to_string(KAO_MAX_RF) + " replicas in a partition");
    for (auto &kv : dense) {
        kv.second = (int)r.broker_id.size();
        r.broker_id.push_back(kv.first);
    }
    r.c.assign(r.P * r.W, KAO_NONE);
    r.t.assign(r.P * r.W, KAO_NONE);
    for (size_t i = 0; i < r.P; ++i) {
        for (size_t j = 0; j < cur[i].second.size(); ++j) r.c[i * r.W + j] = (uint16_t)dense[cur[i].second[j]];
        for (size_t j = 0; j < r.replicas[i].size(); ++j) r.t[i * r.W + j] = (uint16_t)dense[r.replicas[i][j]];
    }
    return r;
}

// The row test: b is a broker and the row does not hold it.  A partition's added brokers are those of its target row that its
// current row lacks, its removed ones those of its current row that its target row lacks.
bool lacks(const uint16_t *row, size_t W, uint16_t b) { return b != KAO_NONE && std::find(row, row + W, b) == row + W; }

// participants of one partition and their copies of it: 1 at each added broker, n_added at the source; empty when it moves no data
std::vector<std::pair<int, uint64_t>> traffic(const uint16_t *c, const uint16_t *t, size_t W) {
    std::vector<std::pair<int, uint64_t>> out;
    for (size_t i = 0; i < W; ++i)
        if (lacks(c, W, t[i])) out.emplace_back(t[i], 1);
    if (!out.empty() && c[0] != KAO_NONE) out.emplace_back(c[0], (uint64_t)out.size());
    return out;
}

// bytes per partition; every partition that moves data needs one
std::vector<uint64_t> partition_sizes(const Options &o, const Rows &r) {
    const std::map<Key, uint64_t> known = o.sizes_path.empty() ? std::map<Key, uint64_t>() : load_sizes(o.sizes_path);
    std::vector<uint64_t> size(std::max<size_t>(r.P, 1), 0);
    std::vector<std::string> missing;
    for (size_t i = 0; i < r.P; ++i) {
        auto it = known.find(r.keys[i]);
        if (it != known.end()) size[i] = it->second;
        else if (!traffic(&r.c[i * r.W], &r.t[i * r.W], r.W).empty()) {
            if (o.have_default) size[i] = o.default_size;
            else missing.push_back(r.keys[i].first + "-" + std::to_string(r.keys[i].second));
        }
    }
    if (!missing.empty()) throw std::runtime_error("no size for moving partitions " + name_list(missing) + " (give them in --sizes or set --default-size)");
    return size;
}

// --headroom, per dense broker: what it holds now, its capacity, and capacity * PCT / 100, which the call takes
struct Disks { std::vector<uint64_t> stored, capacity, effective; };

Disks broker_disks(const Options &o, const Rows &r, const std::vector<uint64_t> &size) {
    Disks d;
    std::map<int, std::vector<LogDir>> dirs;
    if (slurp(o.sizes_path).find("\"brokers\"") != std::string::npos) dirs = load_log_dirs(o.sizes_path);
    const std::map<int, uint64_t> table = o.caps_arg.empty() ? std::map<int, uint64_t>() : read_broker_capacities(o.caps_arg);
    d.stored.assign(r.broker_id.size(), 0);
    for (size_t i = 0; i < r.P; ++i)
        for (size_t j = 0; j < r.W; ++j)
            if (r.c[i * r.W + j] != KAO_NONE) d.stored[r.c[i * r.W + j]] += size[i];
    std::vector<std::string> missing;
    for (size_t b = 0; b < r.broker_id.size(); ++b) {
        uint64_t on_disk = 0, total = 0;
        bool every = false;
        auto bd = dirs.find(r.broker_id[b]);
        if (bd != dirs.end()) {
            every = !bd->second.empty();
            for (auto &ld : bd->second) {
                every = every && ld.has_total;
                total += ld.total_bytes;
                for (auto &e : ld.entries) on_disk += e.size;   // future replicas too: they are bytes on disk
            }
        }
        d.stored[b] = std::max(d.stored[b], on_disk);
        auto it = table.find(r.broker_id[b]);
        if (it != table.end()) d.capacity.push_back(it->second);
        else if (every && total > 0) d.capacity.push_back(total);
        else if (o.have_default_cap) d.capacity.push_back(o.default_cap);
        else missing.push_back(std::to_string(r.broker_id[b]));
    }
    if (!missing.empty())
        throw std::runtime_error("no capacity for brokers " + name_list(missing) +
                                 " (give them in --capacities, read totalBytes from a kafka-log-dirs --sizes document or set --default-capacity)");
    for (uint64_t v : d.capacity) d.effective.push_back((uint64_t)((unsigned __int128)v * (unsigned)o.max_util / 100u));
    return d;
}

// what a call gives back; the plain and the sized call leave stats[] as it is
struct Called {
    std::vector<int32_t> wave;
    int32_t n_waves = 0, lb = 0;
    int64_t stats[8] = {0, 0, -1, 0, 0, -1, -1, -1};
};

// the one call of the library
Called call(const Options &o, const Rows &r, const std::vector<uint64_t> &size, const Disks &d) {
    Called c;
    c.wave.resize(std::max<size_t>(r.P, 1));
    const int32_t B = (int32_t)r.broker_id.size(), P = (int32_t)r.P, W = (int32_t)r.W;
    const char *const name = o.headroom ? "kao_plan_waves_headroom" : o.sized ? "kao_plan_waves_sized" : "kao_plan_waves";
    int rc;
    if (o.headroom)
        rc = kao_plan_waves_headroom(B, P, W, r.c.data(), r.t.data(), size.data(), d.stored.data(), d.effective.data(), o.cap_bytes, o.k, o.seed, c.wave.data(),
                                     &c.n_waves, &c.lb, c.stats);
    else if (o.sized)
        rc = kao_plan_waves_sized(B, P, W, r.c.data(), r.t.data(), size.data(), o.cap_bytes, o.k, o.seed, c.wave.data(), &c.n_waves, &c.lb);
    else
        rc = kao_plan_waves(B, P, W, r.c.data(), r.t.data(), o.k, o.seed, c.wave.data(), &c.n_waves, &c.lb);
    if (rc) throw std::runtime_error(std::string(name) + ": " + kao_strerror(rc) + " " + kao_last_error());
    return c;
}

// the partitions whose wave is `wave_value` as a reassignment document of their own; how many they are
int write_document(const std::string &path, const Rows &r, const std::vector<int32_t> &wave, int32_t wave_value) {
    std::ofstream f(path);
    if (!f) throw std::runtime_error("cannot write " + path);
    f << "{\"version\":1,\"partitions\":[";
    int n = 0;
    for (size_t i = 0; i < r.P; ++i) {
        if (wave[i] != wave_value) continue;
        f << (n++ ? ",\n" : "\n") << "    {\"topic\":" << quoted(r.keys[i].first) << ",\"partition\":" << r.keys[i].second << ",\"replicas\":[";
        for (size_t j = 0; j < r.replicas[i].size(); ++j) f << (j ? "," : "") << r.replicas[i][j];
        f << "]}";
    }
    f << "\n]}\n";
    if (!f) throw std::runtime_error("cannot write " + path);
    return n;
}

// --report, sized: the byte lower bound max_b ceil(sum_p min(t, C) / C) and each wave's busiest broker
void report_bytes(const Options &o, const Rows &r, const std::vector<uint64_t> &size, const Called &c) {
    std::map<std::pair<int, int>, uint64_t> load;
    std::map<int, uint64_t> clamp;
    for (size_t i = 0; i < r.P; ++i)
        for (auto &bn : traffic(&r.c[i * r.W], &r.t[i * r.W], r.W)) {
            const uint64_t tr = bn.second * size[i];   // below 2^62: kao_plan_waves_sized checked the totals
            if (c.wave[i] >= 0) load[{c.wave[i], bn.first}] += tr;   // a stuck partition (--headroom) is in no wave
            if (o.cap_bytes) clamp[bn.first] += std::min(tr, o.cap_bytes);
        }
    uint64_t blb = 0;
    for (auto &kv : clamp) blb = std::max(blb, kv.second / o.cap_bytes + (kv.second % o.cap_bytes != 0));
    std::vector<uint64_t> peak((size_t)c.n_waves, 0);
    for (auto &kv : load) peak[(size_t)kv.first.first] = std::max(peak[(size_t)kv.first.first], kv.second);
    std::fprintf(stderr, " bytes_lower_bound=%llu max_broker_bytes_per_wave=", (unsigned long long)blb);
    for (int w = 0; w < c.n_waves; ++w) std::fprintf(stderr, "%s%llu", w ? "," : "", (unsigned long long)peak[(size_t)w]);
}

// --report, headroom: the fullest receiving broker of each wave in percent of its capacity (occ follows the waves), then the stats
void report_utilisation(const Rows &r, const std::vector<uint64_t> &size, const Disks &d, const Called &c) {
    std::vector<uint64_t> occ = d.stored;
    std::fprintf(stderr, " fullest_receiver_pct_per_wave=");
    for (int w = 0; w < c.n_waves; ++w) {
        std::map<int, uint64_t> arr, dep;
        for (size_t i = 0; i < r.P; ++i) {
            if (c.wave[i] != w || size[i] == 0) continue;
            const uint16_t *cr = &r.c[i * r.W], *tr = &r.t[i * r.W];
            for (size_t j = 0; j < r.W; ++j) {
                if (lacks(cr, r.W, tr[j])) arr[tr[j]] += size[i];
                if (lacks(tr, r.W, cr[j])) dep[cr[j]] += size[i];
            }
        }
        unsigned long long ppm = 0;
        for (auto &kv : arr) {
            const uint64_t cap = d.capacity[(size_t)kv.first];
            const unsigned __int128 v = cap ? (unsigned __int128)(occ[(size_t)kv.first] + kv.second) * 1000000u / cap : 1000000u;
            ppm = std::max(ppm, (unsigned long long)v);
        }
        for (auto &kv : arr) occ[(size_t)kv.first] += kv.second;
        for (auto &kv : dep) occ[(size_t)kv.first] -= kv.second;
        std::fprintf(stderr, "%s%llu.%02llu", w ? "," : "", ppm / 10000, ppm / 100 % 100);
    }
    std::fprintf(stderr, " min_free=%lld min_free_wave=%lld min_free_broker=%d stuck=%lld stuck_bytes=%lld", (long long)c.stats[5],
                 (long long)(c.stats[6] >= 0 ? c.stats[6] + 1 : 0), c.stats[7] >= 0 ? r.broker_id[(size_t)c.stats[7]] : -1, (long long)c.stats[0],
                 (long long)c.stats[1]);
}

// --report: one line to stderr
void report(const Options &o, const Rows &r, const std::vector<uint64_t> &size, const Disks &d, const Called &c, const std::vector<int> &per_wave) {
    std::fprintf(stderr, "waves=%d lower_bound=%d optimal=%s partitions_per_wave=", c.n_waves, c.lb, c.n_waves == c.lb && c.stats[0] == 0 ? "yes" : "no");
    for (int w = 0; w < c.n_waves; ++w) std::fprintf(stderr, "%s%d", w ? "," : "", per_wave[(size_t)w]);
    if (o.sized) report_bytes(o, r, size, c);
    if (o.headroom) report_utilisation(r, size, d, c);
    std::fprintf(stderr, "\n");
}

// documents -> rows -> sizes -> disks -> the call -> wave files -> report; every input error comes before the device is touched.
// The exit status: 3 when partitions are stuck, else 0.
int run(const Options &o) {
    const Rows r = map_documents(o);
    const std::vector<uint64_t> size = o.sized ? partition_sizes(o, r) : std::vector<uint64_t>();
    const Disks d = o.headroom ? broker_disks(o, r, size) : Disks();
    const int rc = kao_init(o.device);
    if (rc) throw std::runtime_error(std::string("kao_init: ") + kao_strerror(rc) + " " + kao_last_error());
    const Called c = call(o, r, size, d);
    std::vector<int> per_wave;
    for (int w = 0; w < c.n_waves; ++w) per_wave.push_back(write_document(o.prefix + std::to_string(w + 1) + ".json", r, c.wave, w));
    if (c.stats[0] > 0) write_document(o.prefix + "-stuck.json", r, c.wave, -2);   // the partitions that fit no wave
    if (o.report) report(o, r, size, d, c, per_wave);
    kao_shutdown();
    if (c.stats[0] > 0) {
        std::fprintf(stderr, "stuck: %lld partitions, %lld bytes\n", (long long)c.stats[0], (long long)c.stats[1]);
        return 3;
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    Options o;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto need = [&](const char *flag) -> std::string { if (i + 1 >= argc) usage((std::string(flag) + " needs a value").c_str()); return argv[++i]; };
        if (a == "--current") o.cur_path = need("--current");
        else if (a == "--plan") o.plan_path = need("--plan");
        else if (a == "--max-per-broker") { o.k = std::atoi(need("--max-per-broker").c_str()); o.have_k = true; }
        else if (a == "--sizes") { o.sizes_path = need("--sizes"); o.sized = true; }
        else if (a == "--max-bytes-per-broker") {
            if (!parse_bytes(need("--max-bytes-per-broker"), o.cap_bytes)) usage("--max-bytes-per-broker needs a byte count (N, or N with K/M/G/T)");
            o.sized = true;
        } else if (a == "--default-size") {
            if (!parse_bytes(need("--default-size"), o.default_size) || o.default_size > kMaxSize) usage("--default-size needs a byte count up to 2^53");
            o.sized = o.have_default = true;
        }
        else if (a == "--headroom") o.headroom = true;
        else if (a == "--capacities") { o.caps_arg = need("--capacities"); o.headroom = true; }
        else if (a == "--default-capacity") {
            if (!parse_bytes(need("--default-capacity"), o.default_cap)) usage("--default-capacity needs a byte count (N, or N with K/M/G/T)");
            o.headroom = o.have_default_cap = true;
        } else if (a == "--max-utilisation") {
            const std::string v = need("--max-utilisation");
            if (v.empty() || v.size() > 3 || v.find_first_not_of("0123456789") != std::string::npos || (o.max_util = std::atoi(v.c_str())) < 1 || o.max_util > 100)
                usage("--max-utilisation needs a percentage 1..100");
            o.headroom = true;
        }
        else if (a == "--out-prefix") o.prefix = need("--out-prefix");
        else if (a == "--seed") o.seed = std::strtoull(need("--seed").c_str(), nullptr, 0);
        else if (a == "--device") o.device = std::atoi(need("--device").c_str());
        else if (a == "--report") o.report = true;
        else if (a == "-h" || a == "--help") usage(nullptr);
        else usage(("unknown flag " + a).c_str());
    }
    if (o.cur_path.empty() || o.plan_path.empty() || o.prefix.empty()) usage("--current, --plan and --out-prefix are required");
    if (o.headroom && o.sizes_path.empty()) usage("--headroom needs --sizes");
    if (o.headroom && o.k < 0) usage("--max-per-broker must be >= 0");
    o.sized = o.sized || o.headroom;
    if (!o.sized && o.k < 1) usage("--max-per-broker needs a value >= 1");
    if (o.sized && !o.headroom && (o.k < 0 || (o.k == 0 && o.cap_bytes == 0)))
        usage(o.have_k ? "--max-per-broker must be >= 0, and a cap must be set (--max-per-broker >= 1 or --max-bytes-per-broker >= 1)"
                       : "give --max-per-broker K >= 1 or --max-bytes-per-broker N >= 1");
    try {
        return run(o);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "kao-waves: %s\n", e.what());
        return 1;
    }
}
