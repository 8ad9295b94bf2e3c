// kao-leaders -- leader-only rebalancing: the fewest preferred-leader changes that put every broker inside the leader band, replica
// sets kept (kao_balance_leaders).
//
//   kao-leaders --current current.json --broker-list 0,1,2 --racks racks.json [--out plan.json] [--slack N] [--auto-slack]
//               [--cluster] [--cluster-lo N] [--cluster-hi N] [--device D] [--report]
//   kao-leaders --current current.json --broker-list 0,1,2 --racks racks.json (--traffic traffic.json | --sizes log-dirs.txt)
//               [--default-weight N] [--min-gain N] [--max-rounds N] [--exchange] [--out plan.json] [--device D] [--report]
//
// writes a reassignment document holding only the partitions whose preferred leader changes; every row is the current row with the
// new leader swapped to the front, so executing it moves no data (kao-waves puts the whole plan into one wave).  Topics are balanced
// one by one; the band is floor / ceil of partitions / brokers per topic, --slack N widens it by N on both sides, --auto-slack takes
// the smallest N >= --slack that is feasible for the topic.  A partition with a replica outside --broker-list is an error: replica
// sets are kept here, moving replicas is kao-cli's job.  --cluster balances the leaders of all topics together instead
// (kao_balance_leaders_cluster): every topic keeps its band (--slack as above), and the largest number of
// partitions any broker leads over the whole cluster is made as low as leader changes alone can make it, or held to --cluster-hi N
// (which implies --cluster), every broker leading at least --cluster-lo N; topics of different RF are padded; --auto-slack is a usage
// error there.  All computation happens in libkao.so on the GPU; the answer is exact.
// --traffic FILE ({"version":1,"partitions":[{"topic":..,"partition":..,"weight":N}]}) or --sizes FILE (kafka-log-dirs --describe
// output, as kao-waves reads it: the partition's size is its weight) weighs the partitions instead (kao_balance_leaders_weighted,
// DESIGN.md section 4k): the traffic a broker leads, over all topics together, is made even by a deterministic descent, and a lower
// bound computed beside it proves the peak optimal where the two meet (status OPTIMAL_PROVEN, else FEASIBLE_BOUND_GAP; exit status
// 0 both times).  --default-weight N weighs the partitions the file does not name (without it they are an error); --min-gain N moves
// a leader only when the gap it closes exceeds N; --max-rounds N stops the descent early.  Combining them with --slack,
// --auto-slack or the --cluster flags is a usage error.  --exchange goes on from the state where no single leader change helps: two
// partitions on one broker pair swap their leaders (kao_balance_leaders_weighted_exchange); the peak is never
// higher than without it, the plan is longer, no data moves; the report gains a line.  It needs --traffic or --sizes.
// Exit status: 0 = ok, 1 = error or a topic is infeasible, 2 = usage.
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
    if (msg) std::fprintf(stderr, "kao-leaders: %s\n", msg);
    std::fprintf(stderr,
        "usage: kao-leaders --current <reassignment.json> --broker-list <id,id,...> --racks <racks.json | id:rack,...>\n"
        "                   [--out <file>] [--slack N] [--auto-slack] [--cluster] [--cluster-lo N] [--cluster-hi N]\n"
        "                   [--device D] [--report]\n"
        "       weighted: --traffic <traffic.json> | --sizes <kafka-log-dirs output> [--default-weight N] [--min-gain N] [--max-rounds N]\n"
        "                 [--exchange]\n"
        "writes the partitions whose preferred leader changes; exit status: 0 = ok, 1 = error or infeasible, 2 = usage\n");
    std::exit(2);
}

struct TopicData {
    std::string name;
    std::vector<int> partition_ids;
    std::vector<uint16_t> current;  // [P * rf]
    int rf = 0;
};

// --cluster: all topics together (kao_balance_leaders_cluster)
int balance_cluster(const Cluster &cl, const std::string &cur_path, const std::string &out_path, int device, int slack, int cluster_lo,
                    int cluster_hi, bool report) {
    const ClusterRows cr = read_rows(cur_path, cl);
    const int P = (int)cr.keys.size(), B = (int)cl.brokers.size(), W = cr.width;
    std::vector<int32_t> topic_of((size_t)std::max(P, 1), 0), sizes;
    for (int p = 0; p < P; ++p) {
        if (p == 0 || cr.keys[(size_t)p].first != cr.keys[(size_t)p - 1].first) sizes.push_back(0);
        topic_of[(size_t)p] = (int32_t)sizes.size() - 1;
        ++sizes.back();
    }
    if (sizes.empty()) sizes.push_back(0);
    std::vector<int32_t> tlo, thi;
    for (int32_t n : sizes) { tlo.push_back(std::max(0, n / B - slack)); thi.push_back((n + B - 1) / B + slack); }
    int rc = kao_init(device);
    if (rc) throw std::runtime_error(std::string("kao_init: ") + kao_strerror(rc) + " " + kao_last_error());
    std::vector<uint16_t> rows = cr.rows;
    int32_t n_changed = 0, before = 0, after = 0, status = 0, stats[8] = {0};
    rc = kao_balance_leaders_cluster(B, P, W, rows.data(), topic_of.data(), (int32_t)sizes.size(), tlo.data(), thi.data(), cluster_lo, cluster_hi, 0,
                                     &n_changed, &before, &after, &status, stats);
    if (rc) throw std::runtime_error(std::string("kao_balance_leaders_cluster: ") + kao_strerror(rc) + " " + kao_last_error());
    const bool ok = status == KAO_STATUS_OPTIMAL_PROVEN;
    if (!ok)
        std::fprintf(stderr, "kao-leaders: no choice of leaders among the replicas meets every topic's band (slack %d) and the cluster band "
                             "(%d units unrouted); try --slack N\n", slack, stats[7]);
    if (report)
        std::fprintf(stderr, "cluster: status=%s peak_before=%d peak_after=%d leader_changes=%d probes=%d phases=%d rounds=%d paths=%d "
                             "longest_path=%d launches=%d pair_nodes=%d unrouted=%d\n", ok ? "OPTIMAL_PROVEN" : "INFEASIBLE_PROVEN", before, after,
                     n_changed, stats[0], stats[1], stats[2], stats[3], stats[4], stats[5], stats[6], stats[7]);
    const std::string text = changed_rows_text(cr, rows, cl.brokers);
    if (out_path.empty()) std::fputs(text.c_str(), stdout);
    else {
        std::ofstream f(out_path);
        f << text;
        if (!f) throw std::runtime_error("cannot write " + out_path);
    }
    kao_shutdown();
    return ok ? 0 : 1;
}

// --traffic / --sizes: all topics together, every partition weighed (kao_balance_leaders_weighted; with --exchange
// kao_balance_leaders_weighted_exchange)
int balance_weighted(const Cluster &cl, const std::string &cur_path, const std::string &out_path, int device, const std::string &traffic_path,
                     const std::string &sizes_path, bool have_default, uint64_t default_weight, uint64_t min_gain, int max_rounds, bool exchange, bool report) {
    const ClusterRows cr = read_rows(cur_path, cl);
    const int P = (int)cr.keys.size(), B = (int)cl.brokers.size(), W = cr.width;
    const std::map<Key, uint64_t> known = traffic_path.empty() ? load_sizes(sizes_path) : load_traffic(traffic_path);
    std::vector<uint64_t> weight((size_t)std::max(P, 1), 0);
    std::vector<std::string> missing;
    for (int p = 0; p < P; ++p) {
        auto it = known.find(cr.keys[(size_t)p]);
        if (it != known.end()) weight[(size_t)p] = it->second;
        else if (have_default) weight[(size_t)p] = default_weight;
        else missing.push_back(cr.keys[(size_t)p].first + "-" + std::to_string(cr.keys[(size_t)p].second));
    }
    if (!missing.empty()) {
        std::string msg = "no weight for partitions ";
        for (size_t i = 0; i < missing.size() && i < 5; ++i) msg += (i ? ", " : "") + missing[i];
        if (missing.size() > 5) msg += " and " + std::to_string(missing.size() - 5) + " more";
        throw std::runtime_error(msg + " (name them in the file or set --default-weight)");
    }
    int rc = kao_init(device);
    if (rc) throw std::runtime_error(std::string("kao_init: ") + kao_strerror(rc) + " " + kao_last_error());
    std::vector<uint16_t> rows = cr.rows;
    int32_t n_changed = 0, status = 0;
    uint64_t before = 0, after = 0, bound = 0;
    int64_t stats[12] = {0};
    rc = (exchange ? kao_balance_leaders_weighted_exchange : kao_balance_leaders_weighted)(B, P, W, rows.data(), weight.data(), min_gain, max_rounds, 0,
                                                                                           &n_changed, &before, &after, &bound, &status, stats);
    if (rc) throw std::runtime_error(std::string(exchange ? "kao_balance_leaders_weighted_exchange: " : "kao_balance_leaders_weighted: ") + kao_strerror(rc) + " " + kao_last_error());
    if (report)
        std::fprintf(stderr, "weighted: status=%s peak_before=%llu peak_after=%llu lower_bound=%llu leader_changes=%d rounds=%lld moves=%lld "
                             "launches=%lld\n", status == KAO_STATUS_OPTIMAL_PROVEN ? "OPTIMAL_PROVEN" : "FEASIBLE_BOUND_GAP",
                     (unsigned long long)before, (unsigned long long)after, (unsigned long long)bound, n_changed, (long long)stats[0],
                     (long long)stats[1], (long long)stats[3]);
    if (report && exchange)
        std::fprintf(stderr, "exchange: rounds=%lld exchanges=%lld proposals=%lld pair_index_entries=%lld\n", (long long)stats[8], (long long)stats[9],
                     (long long)stats[10], (long long)stats[11]);
    const std::string text = changed_rows_text(cr, rows, cl.brokers);
    if (out_path.empty()) std::fputs(text.c_str(), stdout);
    else {
        std::ofstream f(out_path);
        f << text;
        if (!f) throw std::runtime_error("cannot write " + out_path);
    }
    kao_shutdown();
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    std::string cur_path, brokers_csv, racks_arg, out_path;
    int device = 0, slack0 = 0, cluster_lo = 0, cluster_hi = -1;
    bool report = false, auto_slack = false, cluster = false, have_slack = false, have_cluster_lo = false, have_cluster_hi = false;
    std::string traffic_path, sizes_path;
    bool have_traffic = false, have_sizes = false, have_default = false, have_gain = false, have_rounds = false, exchange = false;
    uint64_t default_weight = 0, min_gain = 0;
    int max_rounds = 0;
    auto u64_arg = [](const std::string &v, uint64_t limit, const char *msg) {   // digits only, at most `limit`
        if (v.empty() || v.size() > 20 || v.find_first_not_of("0123456789") != std::string::npos) usage(msg);
        errno = 0;
        const unsigned long long x = std::strtoull(v.c_str(), nullptr, 10);
        if (errno == ERANGE || x > limit) usage(msg);
        return (uint64_t)x;
    };
    auto count_arg = [](const std::string &v, const char *msg) {
        if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos) usage(msg);
        return std::atoi(v.c_str());
    };
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto need = [&](const char *flag) -> std::string { if (i + 1 >= argc) usage((std::string(flag) + " needs a value").c_str()); return argv[++i]; };
        if (a == "--current") cur_path = need("--current");
        else if (a == "--broker-list") brokers_csv = need("--broker-list");
        else if (a == "--racks") racks_arg = need("--racks");
        else if (a == "--out") out_path = need("--out");
        else if (a == "--slack") {
            const std::string v = need("--slack");
            if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos) usage("--slack needs a value >= 0");
            slack0 = std::atoi(v.c_str());
            have_slack = true;
        }
        else if (a == "--auto-slack") auto_slack = true;
        else if (a == "--cluster") cluster = true;
        else if (a == "--cluster-lo") { cluster_lo = count_arg(need("--cluster-lo"), "--cluster-lo needs a value >= 0"); have_cluster_lo = true; }
        else if (a == "--cluster-hi") { cluster_hi = count_arg(need("--cluster-hi"), "--cluster-hi needs a value >= 0"); cluster = have_cluster_hi = true; }
        else if (a == "--traffic") { traffic_path = need("--traffic"); have_traffic = true; }
        else if (a == "--sizes") { sizes_path = need("--sizes"); have_sizes = true; }
        else if (a == "--default-weight") { default_weight = u64_arg(need("--default-weight"), kMaxSize, "--default-weight needs a value 0..2^53"); have_default = true; }
        else if (a == "--min-gain") { min_gain = u64_arg(need("--min-gain"), UINT64_MAX, "--min-gain needs a value 0..2^64-1"); have_gain = true; }
        else if (a == "--max-rounds") { max_rounds = count_arg(need("--max-rounds"), "--max-rounds needs a value >= 0"); have_rounds = true; }
        else if (a == "--exchange") exchange = true;
        else if (a == "--device") device = std::atoi(need("--device").c_str());
        else if (a == "--report") report = true;
        else if (a == "-h" || a == "--help") usage(nullptr);
        else usage(("unknown flag " + a).c_str());
    }
    if (cur_path.empty() || brokers_csv.empty() || racks_arg.empty()) usage("--current, --broker-list and --racks are required");
    const bool weighted = have_traffic || have_sizes;
    if (have_traffic && have_sizes) usage("give one of --traffic and --sizes");
    if (weighted && (have_slack || auto_slack || cluster || have_cluster_lo || have_cluster_hi))
        usage("--traffic / --sizes cannot be combined with --slack, --auto-slack, --cluster, --cluster-lo or --cluster-hi");
    if (!weighted && (have_default || have_gain || have_rounds)) usage("--default-weight, --min-gain and --max-rounds need --traffic or --sizes");
    if (exchange && !weighted) usage("--exchange needs --traffic or --sizes");
    if (cluster_lo && !cluster) usage("--cluster-lo needs --cluster");
    if (cluster && auto_slack) usage("--auto-slack cannot be combined with --cluster");
    if (cluster && cluster_hi >= 0 && cluster_hi < cluster_lo) usage("--cluster-hi must be >= --cluster-lo");
    try {
        const Cluster cl = read_cluster(brokers_csv, racks_arg);
        const std::vector<int> &brokers = cl.brokers;
        if (weighted)
            return balance_weighted(cl, cur_path, out_path, device, traffic_path, sizes_path, have_default, default_weight, min_gain, max_rounds, exchange, report);
        if (cluster) return balance_cluster(cl, cur_path, out_path, device, slack0, cluster_lo, cluster_hi, report);
        const std::map<int, int> &dense = cl.dense;
        const std::vector<uint8_t> &rack_of = cl.rack_of;

        // ---- current assignment: complete rows over the broker list ---------------------------------
        std::string cur_txt = slurp(cur_path);
        JValue doc = JParser(cur_txt).parse();
        const JValue *parts = doc.get("partitions");
        if (!parts || parts->kind != JValue::Arr) throw std::runtime_error("missing \"partitions\" array");
        std::map<std::string, std::map<int, std::vector<int>>> by_topic;
        for (auto &e : parts->arr) {
            const JValue *t = e.get("topic"), *p = e.get("partition"), *r = e.get("replicas");
            if (!t || !p || !r || r->kind != JValue::Arr) throw std::runtime_error("partition entry needs topic/partition/replicas");
            std::vector<int> reps; for (auto &x : r->arr) reps.push_back((int)x.num);
            by_topic[t->str][(int)p->num] = reps;
        }
        std::vector<TopicData> tds;
        for (auto &kv : by_topic) {
            TopicData td; td.name = kv.first;
            for (auto &pr : kv.second) td.rf = std::max(td.rf, (int)pr.second.size());
            for (auto &pr : kv.second) {
                bool complete = (int)pr.second.size() == td.rf;
                for (int b : pr.second) complete = complete && dense.count(b);
                if (!complete)
                    throw std::runtime_error("partition " + td.name + "-" + std::to_string(pr.first) + " has a replica outside --broker-list or fewer replicas than "
                                             "its topic's other partitions: leader-only rebalancing keeps every replica set (use kao-cli to move replicas)");
                td.partition_ids.push_back(pr.first);
                for (int b : pr.second) td.current.push_back((uint16_t)dense.at(b));
            }
            tds.push_back(std::move(td));
        }
        int rc = kao_init(device);
        if (rc) throw std::runtime_error(std::string("kao_init: ") + kao_strerror(rc) + " " + kao_last_error());

        // ---- balance topic by topic, collect the changed rows ---------------------------------------
        int exit_code = 0, n_out = 0;
        std::string body;
        for (auto &td : tds) {
            kao_topic t{};
            const int P = (int)td.partition_ids.size(), B = (int)brokers.size(), RF = td.rf;
            t.n_brokers = B; t.n_racks = (int)cl.rack_names.size(); t.n_partitions = P; t.rf = t.rf_cur = RF;
            t.rack_of = rack_of.data(); t.current = td.current.data();
            t.w[0][0] = 4; t.w[0][1] = 1; t.w[1][0] = 2; t.w[1][1] = 2;
            t.rep_lo = t.rep_hi = t.rack_lo = t.rack_hi = t.prack_lo = t.prack_hi = -1;
            std::vector<uint16_t> rows;
            int32_t n_changed = 0, status = 0, stats[8] = {0};
            int64_t objective = 0;
            int slack = slack0;
            for (;; ++slack) {   // --auto-slack: the smallest slack >= --slack that is feasible
                t.lead_lo = std::max(0, P / B - slack);
                t.lead_hi = (P + B - 1) / B + slack;
                rows = td.current;
                rc = kao_balance_leaders(&t, rows.data(), &n_changed, &objective, &status, stats);
                if (rc) throw std::runtime_error(std::string("kao_balance_leaders: ") + kao_strerror(rc) + " " + kao_last_error());
                if (status == KAO_STATUS_OPTIMAL_PROVEN || !auto_slack || slack > P) break;
            }
            if (status != KAO_STATUS_OPTIMAL_PROVEN) {
                std::fprintf(stderr, "kao-leaders: topic %s: no choice of leaders among the replicas meets the band (slack %d; %d units unrouted); "
                                     "try --slack N or --auto-slack\n", td.name.c_str(), slack, stats[7]);
                exit_code = 1;
            } else {
                for (int p = 0; p < P; ++p) {
                    if (std::equal(rows.begin() + (size_t)p * RF, rows.begin() + (size_t)(p + 1) * RF, td.current.begin() + (size_t)p * RF)) continue;
                    body += (n_out++ ? ",\n" : "\n");
                    body += "    {\"topic\":" + quoted(td.name) + ",\"partition\":" + std::to_string(td.partition_ids[(size_t)p]) + ",\"replicas\":[";
                    for (int k = 0; k < RF; ++k) body += (k ? "," : "") + std::to_string(brokers[rows[(size_t)p * RF + k]]);
                    body += "]}";
                }
            }
            if (report)
                std::fprintf(stderr, "topic %s: status=%s leader_changes=%d objective=%lld slack=%d over_before=%d under_before=%d phases=%d rounds=%d "
                                     "paths=%d longest_path=%d launches=%d\n", td.name.c_str(),
                             status == KAO_STATUS_OPTIMAL_PROVEN ? "OPTIMAL_PROVEN" : "INFEASIBLE_PROVEN", n_changed, (long long)objective, slack,
                             stats[4], stats[5], stats[0], stats[1], stats[2], stats[3], stats[6]);
        }
        const std::string text = "{\"version\":1,\"partitions\":[" + body + "\n]}\n";
        if (out_path.empty()) std::fputs(text.c_str(), stdout);
        else {
            std::ofstream f(out_path);
            f << text;
            if (!f) throw std::runtime_error("cannot write " + out_path);
        }
        kao_shutdown();
        return exit_code;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "kao-leaders: %s\n", e.what());
        return 1;
    }
}
