// kao-failover -- failover-aware follower order: the order of each partition's followers that keeps the peak leader count after a
// broker or a rack failure as low as it can be, with the fewest follower swaps (kao_failover_order).
//
//   kao-failover --current current.json --broker-list 0,1,2 --racks racks.json --scope broker|rack [--dry-run] [--out plan.json]
//                [--report] [--device D]
//                [(--traffic traffic.json | --sizes log-dirs.txt) [--default-weight N] [--min-gain N] [--max-rounds N]]
//
// When a broker or a rack goes down Kafka hands each orphaned partition to the first live replica of its list.  The plan holds only
// the partitions whose followers change places; every row is the current row with two followers swapped, so executing it moves no
// data and changes no preferred leader (kao-waves puts the whole plan into one wave).  The rows of all topics are taken together:
// the load a failure shifts is a cluster quantity.  Partitions that would go offline in a scenario are reported, not an error.
// --dry-run reports and leaves the plan empty.  All computation happens in libkao.so on the GPU; the answer is exact.
// --traffic FILE or --sizes FILE (as kao-leaders reads them) weighs the partitions instead (kao_failover_order_weighted, DESIGN.md
// section 4l): the peak is the traffic a surviving broker leads after the failure, every scenario runs a deterministic descent, and
// a lower bound computed beside it proves the scenario's peak optimal where the two meet.  --default-weight N weighs the partitions
// the file does not name (without it they are an error); --min-gain N changes an heir only when that closes a gap of more than N;
// --max-rounds N stops every scenario's descent early.  The three are usage errors without a file.
// Exit status: 0 = ok, 1 = error, 2 = usage.
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
    if (msg) std::fprintf(stderr, "kao-failover: %s\n", msg);
    std::fprintf(stderr,
        "usage: kao-failover --current <reassignment.json> --broker-list <id,id,...> --racks <racks.json | id:rack,...>\n"
        "                    --scope broker|rack [--dry-run] [--out <file>] [--report] [--device D]\n"
        "       weighted: --traffic <traffic.json> | --sizes <kafka-log-dirs output> [--default-weight N] [--min-gain N] [--max-rounds N]\n"
        "writes the partitions whose followers change places; exit status: 0 = ok, 1 = error, 2 = usage\n");
    std::exit(2);
}

}  // namespace

int main(int argc, char **argv) {
    std::string cur_path, brokers_csv, racks_arg, out_path, scope_arg;
    int device = 0;
    bool report = false, dry_run = false;
    std::string traffic_path, sizes_path;
    bool have_traffic = false, have_sizes = false, have_default = false, have_gain = false, have_rounds = false;
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
        else if (a == "--scope") scope_arg = need("--scope");
        else if (a == "--out") out_path = need("--out");
        else if (a == "--dry-run") dry_run = true;
        else if (a == "--device") device = std::atoi(need("--device").c_str());
        else if (a == "--report") report = true;
        else if (a == "--traffic") { traffic_path = need("--traffic"); have_traffic = true; }
        else if (a == "--sizes") { sizes_path = need("--sizes"); have_sizes = true; }
        else if (a == "--default-weight") { default_weight = u64_arg(need("--default-weight"), kMaxSize, "--default-weight needs a value 0..2^53"); have_default = true; }
        else if (a == "--min-gain") { min_gain = u64_arg(need("--min-gain"), UINT64_MAX, "--min-gain needs a value 0..2^64-1"); have_gain = true; }
        else if (a == "--max-rounds") { max_rounds = count_arg(need("--max-rounds"), "--max-rounds needs a value >= 0"); have_rounds = true; }
        else if (a == "-h" || a == "--help") usage(nullptr);
        else usage(("unknown flag " + a).c_str());
    }
    if (cur_path.empty() || brokers_csv.empty() || racks_arg.empty() || scope_arg.empty()) usage("--current, --broker-list, --racks and --scope are required");
    if (scope_arg != "broker" && scope_arg != "rack") usage("--scope must be broker or rack");
    const int scope = scope_arg == "rack";
    const bool weighted = have_traffic || have_sizes;
    if (have_traffic && have_sizes) usage("give one of --traffic and --sizes");
    if (!weighted && (have_default || have_gain || have_rounds)) usage("--default-weight, --min-gain and --max-rounds need --traffic or --sizes");
    try {
        const Cluster cl = read_cluster(brokers_csv, racks_arg);
        const std::vector<int> &brokers = cl.brokers;
        const std::vector<std::string> &rack_names = cl.rack_names;

        // ---- current assignment: rows of all topics over the broker list, ordered by (topic, partition) ----
        const ClusterRows cr = read_rows(cur_path, cl);
        const std::vector<uint16_t> &cur = cr.rows;
        const int P = (int)cr.keys.size(), B = (int)brokers.size(), W = cr.width;
        std::vector<uint64_t> weight((size_t)std::max(P, 1), 0);
        if (weighted) {
            const std::map<Key, uint64_t> known = traffic_path.empty() ? load_sizes(sizes_path) : load_traffic(traffic_path);
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
        }
        int rc = kao_init(device);
        if (rc) throw std::runtime_error(std::string("kao_init: ") + kao_strerror(rc) + " " + kao_last_error());

        const int G = scope == 0 ? B : (int)rack_names.size();
        std::vector<uint16_t> rows = cur;
        if (weighted) {
            std::vector<uint64_t> scen((size_t)G * 6, 0);
            int32_t n_reordered = 0, status = 0;
            int64_t stats[8] = {0};
            rc = kao_failover_order_weighted(B, (int)rack_names.size(), cl.rack_of.data(), P, W, rows.data(), weight.data(), scope, min_gain, max_rounds,
                                             dry_run ? 1 : 0, scen.data(), &n_reordered, &status, stats);
            if (rc) throw std::runtime_error(std::string("kao_failover_order_weighted: ") + kao_strerror(rc) + " " + kao_last_error());
            if (report) {
                unsigned long long worst_before = 0, worst_after = 0, worst_bound = 0, offline = 0;
                for (int g = 0; g < G; ++g) {
                    const uint64_t *s = &scen[(size_t)g * 6];
                    worst_before = std::max(worst_before, (unsigned long long)s[2]);
                    worst_after = std::max(worst_after, (unsigned long long)s[3]);
                    worst_bound = std::max(worst_bound, (unsigned long long)s[4]);
                    offline += s[1];
                    if (!s[0] && !s[1]) continue;
                    const std::string name = scope == 0 ? std::to_string(brokers[(size_t)g]) : rack_names[(size_t)g];
                    std::fprintf(stderr, "scenario=%s affected=%llu offline=%llu peak_before=%llu peak_after=%llu lower_bound=%llu reordered=%llu\n",
                                 name.c_str(), (unsigned long long)s[0], (unsigned long long)s[1], (unsigned long long)s[2], (unsigned long long)s[3],
                                 (unsigned long long)s[4], (unsigned long long)s[5]);
                }
                std::fprintf(stderr, "weighted: scope=%s scenarios=%d worst_peak_before=%llu worst_peak_after=%llu worst_lower_bound=%llu proven=%lld "
                                     "offline=%llu reordered=%d rounds=%lld moves=%lld launches=%lld\n", scope_arg.c_str(), G, worst_before, worst_after,
                             worst_bound, (long long)stats[6], offline, n_reordered, (long long)stats[1], (long long)stats[2], (long long)stats[4]);
            }
        } else {
            std::vector<int32_t> scen((size_t)G * 5, 0);
            int32_t n_reordered = 0, stats[8] = {0};
            rc = kao_failover_order(B, (int)rack_names.size(), cl.rack_of.data(), P, W, rows.data(), scope, dry_run ? 1 : 0, scen.data(), &n_reordered, stats);
            if (rc) throw std::runtime_error(std::string("kao_failover_order: ") + kao_strerror(rc) + " " + kao_last_error());

            if (report) {
                int worst_before = 0, worst_after = 0;
                long long offline = 0;
                for (int g = 0; g < G; ++g) {
                    const int32_t *s = &scen[(size_t)g * 5];
                    worst_before = std::max(worst_before, (int)s[2]);
                    worst_after = std::max(worst_after, (int)s[3]);
                    offline += s[1];
                    if (!s[0] && !s[1]) continue;
                    const std::string name = scope == 0 ? std::to_string(brokers[(size_t)g]) : rack_names[(size_t)g];
                    std::fprintf(stderr, "scenario=%s affected=%d offline=%d peak_before=%d peak_after=%d reordered=%d\n", name.c_str(), s[0], s[1], s[2], s[3], s[4]);
                }
                std::fprintf(stderr, "scope=%s scenarios=%d worst_peak_before=%d worst_peak_after=%d offline=%lld reordered=%d\n", scope_arg.c_str(), G,
                             worst_before, worst_after, offline, n_reordered);
            }
        }
        const std::string text = changed_rows_text(cr, rows, brokers);
        if (out_path.empty()) std::fputs(text.c_str(), stdout);
        else {
            std::ofstream f(out_path);
            f << text;
            if (!f) throw std::runtime_error("cannot write " + out_path);
        }
        kao_shutdown();
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "kao-failover: %s\n", e.what());
        return 1;
    }
}
