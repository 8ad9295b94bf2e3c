// kao-waves -- split a reassignment plan into waves with at most K partition movements per broker per wave (kao_plan_waves,
// DESIGN.md section 4g).  The pipeline is
//
//   kao-cli --current current.json ... --out plan.json
//   kao-waves --current current.json --plan plan.json --max-per-broker K --out-prefix wave [--seed S] [--device D] [--report]
//
// which writes wave1.json .. waveN.json, each a reassignment document `kafka-reassign-partitions --execute` takes on its own; run
// them in order, each after the previous one has finished.  A partition of current.json that plan.json leaves out is unchanged;
// a partition of plan.json that current.json does not list is an error.  All computation happens in libkao.so on the GPU.
// Exit status: 0 = waves written, 1 = error, 2 = usage.
#include <algorithm>
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../include/kao.h"
#include "kao_json.h"

namespace {

[[noreturn]] void usage(const char *msg) {
    if (msg) std::fprintf(stderr, "kao-waves: %s\n", msg);
    std::fprintf(stderr,
        "usage: kao-waves --current <reassignment.json> --plan <reassignment.json> --max-per-broker K --out-prefix PREFIX\n"
        "                 [--seed S] [--device D] [--report]\n"
        "writes PREFIX1.json .. PREFIXn.json; exit status: 0 = ok, 1 = error, 2 = usage\n");
    std::exit(2);
}

using Key = std::pair<std::string, int>;

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

}  // namespace

int main(int argc, char **argv) {
    std::string cur_path, plan_path, prefix;
    int k = 0, device = 0;
    unsigned long long seed = 1;
    bool report = false;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto need = [&](const char *flag) -> std::string { if (i + 1 >= argc) usage((std::string(flag) + " needs a value").c_str()); return argv[++i]; };
        if (a == "--current") cur_path = need("--current");
        else if (a == "--plan") plan_path = need("--plan");
        else if (a == "--max-per-broker") k = std::atoi(need("--max-per-broker").c_str());
        else if (a == "--out-prefix") prefix = need("--out-prefix");
        else if (a == "--seed") seed = std::strtoull(need("--seed").c_str(), nullptr, 0);
        else if (a == "--device") device = std::atoi(need("--device").c_str());
        else if (a == "--report") report = true;
        else if (a == "-h" || a == "--help") usage(nullptr);
        else usage(("unknown flag " + a).c_str());
    }
    if (cur_path.empty() || plan_path.empty() || prefix.empty()) usage("--current, --plan and --out-prefix are required");
    if (k < 1) usage("--max-per-broker needs a value >= 1");
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
        int rc = kao_init(device);
        if (rc) throw std::runtime_error(std::string("kao_init: ") + kao_strerror(rc) + " " + kao_last_error());
        std::vector<int32_t> wave(std::max<size_t>(P, 1));
        int32_t n_waves = 0, lb = 0;
        rc = kao_plan_waves(nb, (int32_t)P, (int32_t)W, c.data(), t.data(), k, seed, wave.data(), &n_waves, &lb);
        if (rc) throw std::runtime_error(std::string("kao_plan_waves: ") + kao_strerror(rc) + " " + kao_last_error());
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
        if (report) {
            std::fprintf(stderr, "waves=%d lower_bound=%d optimal=%s partitions_per_wave=", n_waves, lb, n_waves == lb ? "yes" : "no");
            for (int w = 0; w < n_waves; ++w) std::fprintf(stderr, "%s%d", w ? "," : "", sizes[(size_t)w]);
            std::fprintf(stderr, "\n");
        }
        kao_shutdown();
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "kao-waves: %s\n", e.what());
        return 1;
    }
}
