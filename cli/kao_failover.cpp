// kao-failover -- failover-aware follower order: the order of each partition's followers that keeps the peak leader count after a
// broker or a rack failure as low as it can be, with the fewest follower swaps (kao_failover_order).
//
//   kao-failover --current current.json --broker-list 0,1,2 --racks racks.json --scope broker|rack [--dry-run] [--out plan.json]
//                [--report] [--device D]
//
// When a broker or a rack goes down Kafka hands each orphaned partition to the first live replica of its list.  The plan holds only
// the partitions whose followers change places; every row is the current row with two followers swapped, so executing it moves no
// data and changes no preferred leader (kao-waves puts the whole plan into one wave).  The rows of all topics are taken together:
// the load a failure shifts is a cluster quantity.  Partitions that would go offline in a scenario are reported, not an error.
// --dry-run reports and leaves the plan empty.  All computation happens in libkao.so on the GPU; the answer is exact.
// Exit status: 0 = ok, 1 = error, 2 = usage.
#include <algorithm>
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

namespace {

[[noreturn]] void usage(const char *msg) {
    if (msg) std::fprintf(stderr, "kao-failover: %s\n", msg);
    std::fprintf(stderr,
        "usage: kao-failover --current <reassignment.json> --broker-list <id,id,...> --racks <racks.json | id:rack,...>\n"
        "                    --scope broker|rack [--dry-run] [--out <file>] [--report] [--device D]\n"
        "writes the partitions whose followers change places; exit status: 0 = ok, 1 = error, 2 = usage\n");
    std::exit(2);
}

}  // namespace

int main(int argc, char **argv) {
    std::string cur_path, brokers_csv, racks_arg, out_path, scope_arg;
    int device = 0;
    bool report = false, dry_run = false;
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
        else if (a == "-h" || a == "--help") usage(nullptr);
        else usage(("unknown flag " + a).c_str());
    }
    if (cur_path.empty() || brokers_csv.empty() || racks_arg.empty() || scope_arg.empty()) usage("--current, --broker-list, --racks and --scope are required");
    if (scope_arg != "broker" && scope_arg != "rack") usage("--scope must be broker or rack");
    const int scope = scope_arg == "rack";
    try {
        const Cluster cl = read_cluster(brokers_csv, racks_arg);
        const std::vector<int> &brokers = cl.brokers;
        const std::vector<std::string> &rack_names = cl.rack_names;

        // ---- current assignment: rows of all topics over the broker list, ordered by (topic, partition) ----
        const ClusterRows cr = read_rows(cur_path, cl);
        const std::vector<uint16_t> &cur = cr.rows;
        const int P = (int)cr.keys.size(), B = (int)brokers.size(), W = cr.width;
        int rc = kao_init(device);
        if (rc) throw std::runtime_error(std::string("kao_init: ") + kao_strerror(rc) + " " + kao_last_error());

        const int G = scope == 0 ? B : (int)rack_names.size();
        std::vector<uint16_t> rows = cur;
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
