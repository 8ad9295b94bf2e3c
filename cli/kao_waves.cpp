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

// participants of one partition and their copies of it: 1 at each added broker, n_added at the source; empty when it moves no data
std::vector<std::pair<int, uint64_t>> traffic(const uint16_t *c, const uint16_t *t, size_t W) {
    std::vector<std::pair<int, uint64_t>> out;
    for (size_t i = 0; i < W; ++i) {
        if (t[i] == KAO_NONE) continue;
        bool held = false;
        for (size_t j = 0; j < W; ++j) held |= c[j] == t[i];
        if (!held) out.emplace_back(t[i], 1);
    }
    if (!out.empty() && c[0] != KAO_NONE) out.emplace_back(c[0], (uint64_t)out.size());
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

}  // namespace

int main(int argc, char **argv) {
    std::string cur_path, plan_path, prefix, sizes_path;
    int k = 0, device = 0;
    unsigned long long seed = 1;
    bool report = false, have_k = false, sized = false, have_default = false, headroom = false, have_default_cap = false;
    uint64_t cap_bytes = 0, default_size = 0, default_cap = 0;
    std::string caps_arg;
    int max_util = 100;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto need = [&](const char *flag) -> std::string { if (i + 1 >= argc) usage((std::string(flag) + " needs a value").c_str()); return argv[++i]; };
        if (a == "--current") cur_path = need("--current");
        else if (a == "--plan") plan_path = need("--plan");
        else if (a == "--max-per-broker") { k = std::atoi(need("--max-per-broker").c_str()); have_k = true; }
        else if (a == "--sizes") { sizes_path = need("--sizes"); sized = true; }
        else if (a == "--max-bytes-per-broker") {
            if (!parse_bytes(need("--max-bytes-per-broker"), cap_bytes)) usage("--max-bytes-per-broker needs a byte count (N, or N with K/M/G/T)");
            sized = true;
        } else if (a == "--default-size") {
            if (!parse_bytes(need("--default-size"), default_size) || default_size > kMaxSize) usage("--default-size needs a byte count up to 2^53");
            sized = have_default = true;
        }
        else if (a == "--headroom") headroom = true;
        else if (a == "--capacities") { caps_arg = need("--capacities"); headroom = true; }
        else if (a == "--default-capacity") {
            if (!parse_bytes(need("--default-capacity"), default_cap)) usage("--default-capacity needs a byte count (N, or N with K/M/G/T)");
            headroom = have_default_cap = true;
        } else if (a == "--max-utilisation") {
            const std::string v = need("--max-utilisation");
            if (v.empty() || v.size() > 3 || v.find_first_not_of("0123456789") != std::string::npos || (max_util = std::atoi(v.c_str())) < 1 || max_util > 100)
                usage("--max-utilisation needs a percentage 1..100");
            headroom = true;
        }
        else if (a == "--out-prefix") prefix = need("--out-prefix");
        else if (a == "--seed") seed = std::strtoull(need("--seed").c_str(), nullptr, 0);
        else if (a == "--device") device = std::atoi(need("--device").c_str());
        else if (a == "--report") report = true;
        else if (a == "-h" || a == "--help") usage(nullptr);
        else usage(("unknown flag " + a).c_str());
    }
    if (cur_path.empty() || plan_path.empty() || prefix.empty()) usage("--current, --plan and --out-prefix are required");
    if (headroom && sizes_path.empty()) usage("--headroom needs --sizes");
    if (headroom && k < 0) usage("--max-per-broker must be >= 0");
    sized = sized || headroom;
    if (!sized && k < 1) usage("--max-per-broker needs a value >= 1");
    if (sized && !headroom && (k < 0 || (k == 0 && cap_bytes == 0)))
        usage(have_k ? "--max-per-broker must be >= 0, and a cap must be set (--max-per-broker >= 1 or --max-bytes-per-broker >= 1)"
                     : "give --max-per-broker K >= 1 or --max-bytes-per-broker N >= 1");
    try {
        const auto cur = entries(cur_path, "current");
        const auto plan = entries(plan_path, "plan");
        std::map<Key, size_t> index;
        for (size_t i = 0; i < cur.size(); ++i) index[cur[i].first] = i;
        std::vector<const std::vector<int> *> tgt(cur.size());
        for (size_t i = 0; i < cur.size(); ++i) tgt[i] = &cur[i].second;
        for (auto &e : plan) {
            auto it = index.find(e.first);
            if (it == index.end())
                throw std::runtime_error("plan names partition " + e.first.first + "-" + std::to_string(e.first.second) + ", which the current assignment does not have");
            tgt[it->second] = &e.second;
        }
        // union broker index: every id of either document, ascending
        std::map<int, int> dense;
        size_t width = 1;
        for (size_t i = 0; i < cur.size(); ++i) {
            for (int b : cur[i].second) dense[b] = 0;
            for (int b : *tgt[i]) dense[b] = 0;
            width = std::max({width, cur[i].second.size(), tgt[i]->size()});
        }
        if (width > KAO_MAX_RF) throw std::runtime_error("more than " + std::to_string(KAO_MAX_RF) + " replicas in a partition");
        int nb = 0;
        for (auto &kv : dense) kv.second = nb++;
        const size_t P = cur.size(), W = width;
        std::vector<uint16_t> c(P * W, KAO_NONE), t(P * W, KAO_NONE);
        for (size_t i = 0; i < P; ++i) {
            for (size_t j = 0; j < cur[i].second.size(); ++j) c[i * W + j] = (uint16_t)dense[cur[i].second[j]];
            for (size_t j = 0; j < tgt[i]->size(); ++j) t[i * W + j] = (uint16_t)dense[(*tgt[i])[j]];
        }
        std::vector<uint64_t> size;
        if (sized) {   // bytes per partition; every partition that moves data needs one
            const std::map<Key, uint64_t> known = sizes_path.empty() ? std::map<Key, uint64_t>() : load_sizes(sizes_path);
            size.assign(std::max<size_t>(P, 1), 0);
            std::vector<std::string> missing;
            for (size_t i = 0; i < P; ++i) {
                auto it = known.find(cur[i].first);
                if (it != known.end()) size[i] = it->second;
                else if (!traffic(&c[i * W], &t[i * W], W).empty()) {
                    if (have_default) size[i] = default_size;
                    else missing.push_back(cur[i].first.first + "-" + std::to_string(cur[i].first.second));
                }
            }
            if (!missing.empty()) {
                std::string msg = "no size for moving partitions ";
                for (size_t i = 0; i < missing.size() && i < 5; ++i) msg += (i ? ", " : "") + missing[i];
                if (missing.size() > 5) msg += " and " + std::to_string(missing.size() - 5) + " more";
                throw std::runtime_error(msg + " (give them in --sizes or set --default-size)");
            }
        }
        std::vector<uint64_t> stored, capacity, effective;   // per dense broker (--headroom)
        std::vector<int> broker_id((size_t)nb);
        for (auto &kv : dense) broker_id[(size_t)kv.second] = kv.first;
        if (headroom) {
            std::map<int, std::vector<LogDir>> dirs;
            if (slurp(sizes_path).find("\"brokers\"") != std::string::npos) dirs = load_log_dirs(sizes_path);
            const std::map<int, uint64_t> table = caps_arg.empty() ? std::map<int, uint64_t>() : read_broker_capacities(caps_arg);
            stored.assign((size_t)nb, 0);
            for (size_t i = 0; i < P; ++i)
                for (size_t j = 0; j < W; ++j)
                    if (c[i * W + j] != KAO_NONE) stored[c[i * W + j]] += size[i];
            std::vector<int> missing;
            for (int b = 0; b < nb; ++b) {
                uint64_t on_disk = 0, total = 0;
                bool every = false;
                auto d = dirs.find(broker_id[(size_t)b]);
                if (d != dirs.end()) {
                    every = !d->second.empty();
                    for (auto &ld : d->second) {
                        every = every && ld.has_total;
                        total += ld.total_bytes;
                        for (auto &e : ld.entries) on_disk += e.size;   // future replicas too: they are bytes on disk
                    }
                }
                stored[(size_t)b] = std::max(stored[(size_t)b], on_disk);
                auto it = table.find(broker_id[(size_t)b]);
                if (it != table.end()) capacity.push_back(it->second);
                else if (every && total > 0) capacity.push_back(total);
                else if (have_default_cap) capacity.push_back(default_cap);
                else missing.push_back(broker_id[(size_t)b]);
            }
            if (!missing.empty()) {
                std::string msg = "no capacity for brokers ";
                for (size_t i = 0; i < missing.size() && i < 5; ++i) msg += (i ? ", " : "") + std::to_string(missing[i]);
                if (missing.size() > 5) msg += " and " + std::to_string(missing.size() - 5) + " more";
                throw std::runtime_error(msg + " (give them in --capacities, read totalBytes from a kafka-log-dirs --sizes document or set --default-capacity)");
            }
            for (uint64_t v : capacity) effective.push_back((uint64_t)((unsigned __int128)v * (unsigned)max_util / 100u));
        }
        int rc = kao_init(device);
        if (rc) throw std::runtime_error(std::string("kao_init: ") + kao_strerror(rc) + " " + kao_last_error());
        std::vector<int32_t> wave(std::max<size_t>(P, 1));
        int32_t n_waves = 0, lb = 0;
        int64_t hstats[8] = {0, 0, -1, 0, 0, -1, -1, -1};
        if (headroom) {
            rc = kao_plan_waves_headroom(nb, (int32_t)P, (int32_t)W, c.data(), t.data(), size.data(), stored.data(), effective.data(), cap_bytes, k, seed,
                                         wave.data(), &n_waves, &lb, hstats);
            if (rc) throw std::runtime_error(std::string("kao_plan_waves_headroom: ") + kao_strerror(rc) + " " + kao_last_error());
        } else if (sized) {
            rc = kao_plan_waves_sized(nb, (int32_t)P, (int32_t)W, c.data(), t.data(), size.data(), cap_bytes, k, seed, wave.data(), &n_waves, &lb);
            if (rc) throw std::runtime_error(std::string("kao_plan_waves_sized: ") + kao_strerror(rc) + " " + kao_last_error());
        } else {
            rc = kao_plan_waves(nb, (int32_t)P, (int32_t)W, c.data(), t.data(), k, seed, wave.data(), &n_waves, &lb);
            if (rc) throw std::runtime_error(std::string("kao_plan_waves: ") + kao_strerror(rc) + " " + kao_last_error());
        }
        std::vector<int> sizes((size_t)n_waves, 0);
        for (int w = 0; w < n_waves; ++w) {
            const std::string path = prefix + std::to_string(w + 1) + ".json";
            std::ofstream f(path);
            if (!f) throw std::runtime_error("cannot write " + path);
            f << "{\"version\":1,\"partitions\":[";
            for (size_t i = 0; i < P; ++i) {
                if (wave[i] != w) continue;
                f << (sizes[(size_t)w]++ ? ",\n" : "\n") << "    {\"topic\":" << quoted(cur[i].first.first) << ",\"partition\":" << cur[i].first.second << ",\"replicas\":[";
                for (size_t j = 0; j < tgt[i]->size(); ++j) f << (j ? "," : "") << (*tgt[i])[j];
                f << "]}";
            }
            f << "\n]}\n";
            if (!f) throw std::runtime_error("cannot write " + path);
        }
        if (hstats[0] > 0) {   // the partitions that fit no wave, as a reassignment document of their own
            const std::string path = prefix + "-stuck.json";
            std::ofstream f(path);
            if (!f) throw std::runtime_error("cannot write " + path);
            f << "{\"version\":1,\"partitions\":[";
            bool first = true;
            for (size_t i = 0; i < P; ++i) {
                if (wave[i] != -2) continue;
                f << (first ? "\n" : ",\n") << "    {\"topic\":" << quoted(cur[i].first.first) << ",\"partition\":" << cur[i].first.second << ",\"replicas\":[";
                first = false;
                for (size_t j = 0; j < tgt[i]->size(); ++j) f << (j ? "," : "") << (*tgt[i])[j];
                f << "]}";
            }
            f << "\n]}\n";
            if (!f) throw std::runtime_error("cannot write " + path);
        }
        if (report) {
            std::fprintf(stderr, "waves=%d lower_bound=%d optimal=%s partitions_per_wave=", n_waves, lb, n_waves == lb && hstats[0] == 0 ? "yes" : "no");
            for (int w = 0; w < n_waves; ++w) std::fprintf(stderr, "%s%d", w ? "," : "", sizes[(size_t)w]);
            if (sized) {   // bytes: the byte lower bound max_b ceil(sum_p min(t, C) / C) and each wave's busiest broker
                std::map<std::pair<int, int>, uint64_t> load;
                std::map<int, uint64_t> clamp;
                for (size_t i = 0; i < P; ++i)
                    for (auto &bn : traffic(&c[i * W], &t[i * W], W)) {
                        const uint64_t tr = bn.second * size[i];   // below 2^62: kao_plan_waves_sized checked the totals
                        if (wave[i] >= 0) load[{wave[i], bn.first}] += tr;   // a stuck partition (--headroom) is in no wave
                        if (cap_bytes) clamp[bn.first] += std::min(tr, cap_bytes);
                    }
                uint64_t blb = 0;
                for (auto &kv : clamp) blb = std::max(blb, kv.second / cap_bytes + (kv.second % cap_bytes != 0));
                std::vector<uint64_t> peak((size_t)n_waves, 0);
                for (auto &kv : load) peak[(size_t)kv.first.first] = std::max(peak[(size_t)kv.first.first], kv.second);
                std::fprintf(stderr, " bytes_lower_bound=%llu max_broker_bytes_per_wave=", (unsigned long long)blb);
                for (int w = 0; w < n_waves; ++w) std::fprintf(stderr, "%s%llu", w ? "," : "", (unsigned long long)peak[(size_t)w]);
            }
            if (headroom) {   // the fullest receiving broker of each wave in percent of its capacity: occ follows the waves
                std::vector<uint64_t> occ = stored;
                std::fprintf(stderr, " fullest_receiver_pct_per_wave=");
                for (int w = 0; w < n_waves; ++w) {
                    std::map<int, uint64_t> arr, dep;
                    for (size_t i = 0; i < P; ++i) {
                        if (wave[i] != w || size[i] == 0) continue;
                        for (size_t j = 0; j < W; ++j) {
                            const uint16_t tb = t[i * W + j], cb = c[i * W + j];
                            if (tb != KAO_NONE && std::find(&c[i * W], &c[i * W] + W, tb) == &c[i * W] + W) arr[tb] += size[i];
                            if (cb != KAO_NONE && std::find(&t[i * W], &t[i * W] + W, cb) == &t[i * W] + W) dep[cb] += size[i];
                        }
                    }
                    unsigned long long ppm = 0;
                    for (auto &kv : arr) {
                        const uint64_t cap = capacity[(size_t)kv.first];
                        const unsigned __int128 v = cap ? (unsigned __int128)(occ[(size_t)kv.first] + kv.second) * 1000000u / cap : 1000000u;
                        ppm = std::max(ppm, (unsigned long long)v);
                    }
                    for (auto &kv : arr) occ[(size_t)kv.first] += kv.second;
                    for (auto &kv : dep) occ[(size_t)kv.first] -= kv.second;
                    std::fprintf(stderr, "%s%llu.%02llu", w ? "," : "", ppm / 10000, ppm / 100 % 100);
                }
                std::fprintf(stderr, " min_free=%lld min_free_wave=%lld min_free_broker=%d stuck=%lld stuck_bytes=%lld", (long long)hstats[5],
                             (long long)(hstats[6] >= 0 ? hstats[6] + 1 : 0), hstats[7] >= 0 ? broker_id[(size_t)hstats[7]] : -1, (long long)hstats[0],
                             (long long)hstats[1]);
            }
            std::fprintf(stderr, "\n");
        }
        kao_shutdown();
        if (hstats[0] > 0) {
            std::fprintf(stderr, "stuck: %lld partitions, %lld bytes\n", (long long)hstats[0], (long long)hstats[1]);
            return 3;
        }
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "kao-waves: %s\n", e.what());
        return 1;
    }
}
