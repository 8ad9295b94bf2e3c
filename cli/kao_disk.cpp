// kao-disk -- disk-usage balance: the replica moves that lower the peak of the bytes a broker stores (kao_balance_disk, DESIGN.md
// section 4m; under --max-bytes kao_balance_disk_budget, section 4n; with --capacities kao_balance_disk_capacity, section 4q; with
// --exchange kao_balance_disk_exchange, section 4u; with --drain kao_balance_disk_drain, section 4w; with --replica-band or
// --count-slack kao_balance_disk_banded, section 4x).
//
//   kao-disk --current current.json --broker-list 0,1,2 --racks racks.json --sizes log-dirs.txt [--default-size N]
//            [--max-per-rack N] [--keep-leaders] [--min-gain BYTES] [--max-bytes BYTES] [--max-rounds N] [--dry-run] --out plan.json
//            [--capacities caps.json | id:bytes,...] [--default-capacity BYTES] [--exchange] [--drain ID[,ID...]] [--report] [--device D]
//            [--replica-band LO:HI | --count-slack K]
//
// Every other planner counts a replica as one unit or moves no data; this one reads the partition sizes (`kafka-log-dirs --describe`
// output or a sizes document, as kao-waves reads them) and moves replicas to brokers outside their row until no single move closes a
// gap of more than --min-gain bytes (N, or N with K/M/G/T).  A move keeps its slot, so the follower order stays; --keep-leaders keeps
// every preferred leader where it is; --max-per-rack N lets no move raise a partition's count in a rack above N (counts already
// above it may stay).  The rows of all topics are taken together over one broker index.  --default-size N sizes the partitions the
// file does not name (without it they are an error).  The answer is a deterministic descent with a lower bound beside it: where
// peak_after == lower_bound the peak is proven optimal.  The plan holds the changed rows only and is what kao-waves --plan takes;
// --dry-run reports and leaves the plan empty.  --max-bytes N caps the bytes the whole plan copies: a move that would copy more than
// what is left of N is no candidate, and of a round's winners the heaviest sources are served first; the report line then ends in
// max_bytes, bytes_left, refused (winners the budget turned down) and budget_bound (1: the budget is what stopped the descent).
// --capacities (a JSON file {"<brokerId>": bytes} or id:bytes,id:bytes; a value is a number or a string with K/M/G/T) gives every
// broker its disk size, --default-capacity N that of the brokers the table does not name; a broker of --broker-list without either
// is a usage error.  The moves then lower the peak UTILISATION S(b) / capacity(b), the answer for brokers with unequal disks, and the
// report line ends in peak_before_ppm, peak_after_ppm, lower_bound_ppm (parts per million, rounded down) and thorough_rounds.
// --exchange goes on from the move-stable state with exchanges: two replicas of different partitions trade places across a broker
// pair.  It works by bytes only, so it is refused together with --max-bytes, --capacities or --default-capacity; the report line then
// ends in peak_of_moves (the peak the moves alone reach), exchange_rounds, exchanges and exchange_proposals.
// --drain ID[,ID...] names brokers of --broker-list that are to end empty: their replicas leave whatever the gain (slot 0 and size 0
// included), nothing moves onto them, and the live brokers are balanced around what arrives.  An id outside the list, a duplicate or
// every broker is a usage error.  It works by bytes only, so it is refused together with --max-bytes, --capacities, --default-capacity
// or --exchange.  The report line then ends in draining, drain_bytes_before, drain_bytes_after, drain_moves, last_drain_round,
// replicas_left and bytes_left, and one line "disk: left <topic>-<partition> broker=<id> reason=<why>" follows per replica left: its row
// holds every live broker, the rack rule forbids every other one, or (only when --max-rounds stopped the call) max_rounds.
// --replica-band LO:HI keeps the number of replicas per broker inside LO..HI while the bytes are balanced: no move goes onto a broker
// that holds HI replicas or leaves one that holds LO, so a broker outside the band may move toward it and never away.  --count-slack K
// is the band floor(R/B) - K : ceil(R/B) + K (LO not below 0) for the R replicas on the B brokers of --broker-list.  With --exchange
// the exchanges, which keep every count, go on under the band.  By bytes only: refused together with --max-bytes, --capacities,
// --default-capacity or --drain, and the two flags refuse each other.  The report gains one line "disk: replica_band=LO:HI
// counts_before=MIN..MAX counts_after=MIN..MAX outside_before=N outside_after=N"; a broker outside the band at the end is a warning on
// stderr and exit status 0: the band never forced anything.
// All computation happens in libkao.so on the GPU.
// Exit status: 0 = ok, 1 = error, 2 = usage, 3 = with --drain, replicas are left on a draining broker (every file is written).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "../include/kao.h"
#include "kao_cluster.h"
#include "kao_json.h"
#include "kao_sizes.h"

namespace {

[[noreturn]] void usage(const char *msg) {
    if (msg) std::fprintf(stderr, "kao-disk: %s\n", msg);
    std::fprintf(stderr,
        "usage: kao-disk --current <reassignment.json> --broker-list <id,id,...> --racks <racks.json | id:rack,...>\n"
        "                --sizes <kafka-log-dirs output | sizes.json> [--default-size N] [--max-per-rack N] [--keep-leaders]\n"
        "                [--min-gain N[K|M|G|T]] [--max-bytes N[K|M|G|T]] [--max-rounds N] [--dry-run] --out <file> [--report]\n"
        "                [--capacities <caps.json | id:bytes,...>] [--default-capacity N[K|M|G|T]] [--exchange] [--drain ID[,ID...]]\n"
        "                [--replica-band LO:HI | --count-slack K] [--device D]\n"
        "--exchange: exchanges of two replicas across a broker pair go on from the move-stable state (by bytes only: not with\n"
        "            --max-bytes, --capacities or --default-capacity)\n"
        "--drain: the named brokers of --broker-list are to end empty (by bytes only: not with --max-bytes, --capacities,\n"
        "            --default-capacity or --exchange)\n"
        "--replica-band, --count-slack: the replicas per broker stay inside LO..HI, or within K of the mean (by bytes only: not with\n"
        "            --max-bytes, --capacities, --default-capacity or --drain; with or without --exchange)\n"
        "writes the partitions whose replicas move; exit status: 0 = ok, 1 = error, 2 = usage, 3 = with --drain, replicas are left\n"
        "on a draining broker (no admissible live broker takes them; every file is written)\n");
    std::exit(2);
}

// floor(num * 10^6 / den) in decimal; the product passes 64 bits
std::string ppm(uint64_t num, uint64_t den) {
    unsigned __int128 v = (unsigned __int128)num * 1000000u / den;
    std::string s;
    do { s.insert(s.begin(), (char)('0' + (int)(v % 10))); v /= 10; } while (v);
    return s;
}

}  // namespace

int main(int argc, char **argv) {
    std::string cur_path, brokers_csv, racks_arg, out_path, sizes_path, caps_arg, drain_csv;
    int device = 0, max_per_rack = 0, max_rounds = 0, band_lo = 0, band_hi = 0, slack = 0;
    bool have_band = false, have_slack = false;
    bool report = false, dry_run = false, keep_leaders = false, have_default = false, have_budget = false, have_caps = false, have_default_cap = false, exchange = false, have_drain = false;
    uint64_t default_size = 0, min_gain = 0, max_bytes = 0, default_cap = 0;
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
        else if (a == "--sizes") sizes_path = need("--sizes");
        else if (a == "--out") out_path = need("--out");
        else if (a == "--dry-run") dry_run = true;
        else if (a == "--keep-leaders") keep_leaders = true;
        else if (a == "--exchange") exchange = true;
        else if (a == "--drain") { drain_csv = need("--drain"); have_drain = true; }
        else if (a == "--replica-band") {
            const std::string v = need("--replica-band");
            const size_t at = v.find(':');
            if (at == std::string::npos) usage("--replica-band needs LO:HI, two counts");
            band_lo = count_arg(v.substr(0, at), "--replica-band needs LO:HI, two counts");
            band_hi = count_arg(v.substr(at + 1), "--replica-band needs LO:HI, two counts");
            have_band = true;
        } else if (a == "--count-slack") { slack = count_arg(need("--count-slack"), "--count-slack needs a count"); have_slack = true; }
        else if (a == "--device") device = std::atoi(need("--device").c_str());
        else if (a == "--report") report = true;
        else if (a == "--default-size") {
            if (!parse_bytes(need("--default-size"), default_size) || default_size > kMaxSize) usage("--default-size needs a byte count up to 2^53");
            have_default = true;
        } else if (a == "--min-gain") {
            if (!parse_bytes(need("--min-gain"), min_gain)) usage("--min-gain needs a byte count (N, or N with K/M/G/T)");
        } else if (a == "--max-bytes") {
            if (!parse_bytes(need("--max-bytes"), max_bytes)) usage("--max-bytes needs a byte count (N, or N with K/M/G/T)");
            have_budget = true;
        } else if (a == "--capacities") {
            caps_arg = need("--capacities");
            have_caps = true;
        } else if (a == "--default-capacity") {
            if (!parse_bytes(need("--default-capacity"), default_cap)) usage("--default-capacity needs a byte count (N, or N with K/M/G/T)");
            have_default_cap = true;
        } else if (a == "--max-per-rack") max_per_rack = count_arg(need("--max-per-rack"), "--max-per-rack needs a value >= 0");
        else if (a == "--max-rounds") max_rounds = count_arg(need("--max-rounds"), "--max-rounds needs a value >= 0");
        else if (a == "-h" || a == "--help") usage(nullptr);
        else usage(("unknown flag " + a).c_str());
    }
    if (cur_path.empty() || brokers_csv.empty() || racks_arg.empty() || sizes_path.empty() || out_path.empty())
        usage("--current, --broker-list, --racks, --sizes and --out are required");
    const bool by_capacity = have_caps || have_default_cap;
    if (exchange && (have_budget || by_capacity)) usage("--exchange works by bytes only: not together with --max-bytes, --capacities or --default-capacity");
    if (have_drain && (exchange || have_budget || by_capacity)) usage("--drain works by bytes only: not together with --max-bytes, --capacities, --default-capacity or --exchange");
    if (have_band && (have_budget || by_capacity || have_drain)) usage("--replica-band works by bytes only: not together with --max-bytes, --capacities, --default-capacity or --drain");
    if (have_slack && (have_budget || by_capacity || have_drain)) usage("--count-slack works by bytes only: not together with --max-bytes, --capacities, --default-capacity or --drain");
    if (have_band && have_slack) usage("--replica-band and --count-slack: give one of the two");
    if (have_band && band_hi < band_lo) usage("--replica-band: HI is below LO");
    const bool banded = have_band || have_slack;
    std::vector<uint8_t> drain;       // per broker of --broker-list, in its order: != 0 for a draining one
    if (have_drain) {                 // an unknown id, a duplicate or every broker is a usage error
        std::vector<int> ids;
        for (auto &t : split(brokers_csv, ',')) if (!t.empty()) ids.push_back(std::atoi(t.c_str()));
        drain.assign(ids.size(), 0);
        size_t n = 0;
        for (auto &t : split(drain_csv, ',')) {
            if (t.empty()) continue;
            if (t.size() > 9 || t.find_first_not_of("0123456789") != std::string::npos) usage("--drain needs broker ids, CSV");
            const auto at = std::find(ids.begin(), ids.end(), std::atoi(t.c_str()));
            if (at == ids.end()) usage(("--drain: broker " + t + " is not in the broker list").c_str());
            if (drain[(size_t)(at - ids.begin())]) usage(("--drain: broker " + t + " is named twice").c_str());
            drain[(size_t)(at - ids.begin())] = 1;
            ++n;
        }
        if (n == 0) usage("--drain needs broker ids, CSV");
        if (n == ids.size()) usage("--drain: every broker is draining, no live broker is left");
    }
    std::vector<uint64_t> capacity;   // per broker of --broker-list, in its order
    if (by_capacity) {                // a broker without a capacity is a usage error
        std::string msg;
        try {
            const std::map<int, uint64_t> table = have_caps ? read_broker_capacities(caps_arg) : std::map<int, uint64_t>();
            std::vector<std::string> missing;
            for (auto &t : split(brokers_csv, ',')) {
                if (t.empty()) continue;
                auto it = table.find(std::atoi(t.c_str()));
                if (it != table.end()) capacity.push_back(it->second);
                else if (have_default_cap) capacity.push_back(default_cap);
                else missing.push_back(std::to_string(std::atoi(t.c_str())));
            }
            if (!missing.empty()) {
                msg = "no capacity for brokers ";
                for (size_t i = 0; i < missing.size() && i < 5; ++i) msg += (i ? ", " : "") + missing[i];
                if (missing.size() > 5) msg += " and " + std::to_string(missing.size() - 5) + " more";
                msg += " (give them in --capacities or set --default-capacity)";
            }
        } catch (const std::exception &e) {
            msg = std::string("--capacities: ") + e.what();
        }
        if (!msg.empty()) usage(msg.c_str());
    }
    try {
        const Cluster cl = read_cluster(brokers_csv, racks_arg);
        const ClusterRows cr = read_rows(cur_path, cl);
        const int P = (int)cr.keys.size(), B = (int)cl.brokers.size(), W = cr.width;
        std::vector<uint64_t> size((size_t)std::max(P, 1), 0);
        {
            const std::map<Key, uint64_t> known = load_sizes(sizes_path);
            std::vector<std::string> missing;
            for (int p = 0; p < P; ++p) {
                auto it = known.find(cr.keys[(size_t)p]);
                if (it != known.end()) size[(size_t)p] = it->second;
                else if (have_default) size[(size_t)p] = default_size;
                else missing.push_back(cr.keys[(size_t)p].first + "-" + std::to_string(cr.keys[(size_t)p].second));
            }
            if (!missing.empty()) {
                std::string msg = "no size for partitions ";
                for (size_t i = 0; i < missing.size() && i < 5; ++i) msg += (i ? ", " : "") + missing[i];
                if (missing.size() > 5) msg += " and " + std::to_string(missing.size() - 5) + " more";
                throw std::runtime_error(msg + " (give them in --sizes or set --default-size)");
            }
        }
        int rc = kao_init(device);
        if (rc) throw std::runtime_error(std::string("kao_init: ") + kao_strerror(rc) + " " + kao_last_error());

        std::vector<uint16_t> rows = cr.rows;
        int32_t n_moved = 0, status = 0, n_left = 0;
        uint64_t bytes_left = 0, bytes_moved = 0, before = 0, after = 0, bound = 0, before2[2] = {0, 1}, after2[2] = {0, 1}, bound2[2] = {0, 1};
        int32_t counts[4] = {0, 0, 0, 0};
        int64_t stats[14] = {0};
        if (have_slack && B > 0) {   // floor(R / B) - K : ceil(R / B) + K over the replicas of the rows
            long long R = 0;
            for (uint16_t b : cr.rows) R += b != KAO_NONE;
            band_lo = (int)std::max(0ll, R / B - slack);
            band_hi = (int)std::min((R + B - 1) / B + slack, (long long)INT32_MAX);
        }
        const char *entry = banded ? "kao_balance_disk_banded: " : by_capacity ? "kao_balance_disk_capacity: " : have_budget ? "kao_balance_disk_budget: " : exchange ? "kao_balance_disk_exchange: "
                            : have_drain ? "kao_balance_disk_drain: " : "kao_balance_disk: ";
        if (banded)
            rc = kao_balance_disk_banded(B, (int)cl.rack_names.size(), cl.rack_of.data(), P, W, rows.data(), size.data(), band_lo, band_hi, exchange ? 1 : 0, max_per_rack,
                                         keep_leaders ? 0 : 1, min_gain, max_rounds, dry_run ? 1 : 0, &n_moved, &bytes_moved, &before, &after, &bound, counts, &status, stats);
        else if (by_capacity) {
            rc = kao_balance_disk_capacity(B, (int)cl.rack_names.size(), cl.rack_of.data(), P, W, rows.data(), size.data(), capacity.data(), max_per_rack,
                                           keep_leaders ? 0 : 1, min_gain, have_budget ? max_bytes : UINT64_MAX, max_rounds, dry_run ? 1 : 0, &n_moved,
                                           &bytes_moved, before2, after2, bound2, &status, stats);
            before = before2[0]; after = after2[0]; bound = bound2[0];
        } else if (have_budget)
            rc = kao_balance_disk_budget(B, (int)cl.rack_names.size(), cl.rack_of.data(), P, W, rows.data(), size.data(), max_per_rack, keep_leaders ? 0 : 1,
                                         min_gain, max_bytes, max_rounds, dry_run ? 1 : 0, &n_moved, &bytes_moved, &before, &after, &bound, &status, stats);
        else if (exchange)
            rc = kao_balance_disk_exchange(B, (int)cl.rack_names.size(), cl.rack_of.data(), P, W, rows.data(), size.data(), max_per_rack, keep_leaders ? 0 : 1,
                                           min_gain, max_rounds, dry_run ? 1 : 0, &n_moved, &bytes_moved, &before, &after, &bound, &status, stats);
        else if (have_drain)
            rc = kao_balance_disk_drain(B, (int)cl.rack_names.size(), cl.rack_of.data(), P, W, rows.data(), size.data(), drain.data(), max_per_rack, keep_leaders ? 0 : 1,
                                        min_gain, max_rounds, dry_run ? 1 : 0, &n_moved, &bytes_moved, &before, &after, &bound, &n_left, &bytes_left, &status, stats);
        else
            rc = kao_balance_disk(B, (int)cl.rack_names.size(), cl.rack_of.data(), P, W, rows.data(), size.data(), max_per_rack, keep_leaders ? 0 : 1, min_gain,
                                  max_rounds, dry_run ? 1 : 0, &n_moved, &bytes_moved, &before, &after, &bound, &status, stats);
        if (rc) throw std::runtime_error(std::string(entry) + kao_strerror(rc) + " " + kao_last_error());
        if (report) {
            static const char *const terms[4] = {"largest_partition", "mean_load", "fixed_leaders", "integrality"};
            unsigned long long total = 0;
            for (int p = 0; p < P; ++p)
                for (int j = 0; j < W && cr.rows[(size_t)p * W + j] != KAO_NONE; ++j) total += size[(size_t)p];
            std::fprintf(stderr, "disk: status=%s peak_before=%llu peak_after=%llu lower_bound=%llu bound_term=%s replicas_moved=%d bytes_moved=%llu "
                                 "bytes_total=%llu rows_changed=%lld brokers_changed=%lld rounds=%lld moves=%lld launches=%lld",
                         status == KAO_STATUS_OPTIMAL_PROVEN ? "OPTIMAL_PROVEN" : "FEASIBLE_BOUND_GAP", (unsigned long long)before, (unsigned long long)after,
                         (unsigned long long)bound, terms[stats[6] >= 0 && stats[6] < 4 ? stats[6] : 0], n_moved, (unsigned long long)bytes_moved, total,
                         (long long)stats[4], (long long)stats[7], (long long)stats[0], (long long)stats[1], (long long)stats[3]);
            if (have_budget)
                std::fprintf(stderr, " max_bytes=%llu bytes_left=%llu refused=%lld budget_bound=%lld", (unsigned long long)max_bytes,
                             (unsigned long long)(max_bytes - bytes_moved), (long long)stats[8], (long long)stats[9]);
            if (by_capacity)
                std::fprintf(stderr, " peak_before_ppm=%s peak_after_ppm=%s lower_bound_ppm=%s thorough_rounds=%lld", ppm(before2[0], before2[1]).c_str(),
                             ppm(after2[0], after2[1]).c_str(), ppm(bound2[0], bound2[1]).c_str(), (long long)stats[10]);
            if (exchange)
                std::fprintf(stderr, " peak_of_moves=%lld exchange_rounds=%lld exchanges=%lld exchange_proposals=%lld", (long long)stats[11], (long long)stats[8],
                             (long long)stats[9], (long long)stats[10]);
            if (have_drain) {
                std::string ids;
                unsigned long long held = 0;
                for (int b = 0; b < B; ++b)
                    if (drain[(size_t)b]) ids += (ids.empty() ? "" : ",") + std::to_string(cl.brokers[(size_t)b]);
                for (int p = 0; p < P; ++p)
                    for (int j = 0; j < W && cr.rows[(size_t)p * W + j] != KAO_NONE; ++j) held += drain[cr.rows[(size_t)p * W + j]] ? size[(size_t)p] : 0;
                std::fprintf(stderr, " draining=%s drain_bytes_before=%llu drain_bytes_after=%llu drain_moves=%lld last_drain_round=%lld replicas_left=%d bytes_left=%llu",
                             ids.c_str(), held, (unsigned long long)bytes_left, (long long)stats[8], (long long)stats[9], n_left, (unsigned long long)bytes_left);
            }
            std::fprintf(stderr, "\n");
            if (banded)
                std::fprintf(stderr, "disk: replica_band=%d:%d counts_before=%d..%d counts_after=%d..%d outside_before=%lld outside_after=%lld\n", band_lo, band_hi, counts[0],
                             counts[1], counts[2], counts[3], (long long)stats[13], (long long)stats[12]);
            for (int p = 0; have_drain && !dry_run && p < P; ++p) {   // one line per replica left, by row and slot, with the reason
                const uint16_t *row = rows.data() + (size_t)p * W;
                int k = 0;
                while (k < W && row[k] != KAO_NONE) ++k;
                for (int j = 0; j < k; ++j) {
                    if (!drain[row[j]]) continue;
                    bool outside = false, ok = false;
                    for (int c = 0; c < B; ++c) {
                        if (drain[(size_t)c] || std::find(row, row + k, (uint16_t)c) != row + k) continue;
                        outside = true;
                        int cnt = 0;
                        for (int i = 0; i < k; ++i) cnt += cl.rack_of[row[i]] == cl.rack_of[(size_t)c];
                        ok |= max_per_rack <= 0 || cl.rack_of[(size_t)c] == cl.rack_of[row[j]] || cnt < max_per_rack;
                    }
                    std::fprintf(stderr, "disk: left %s-%d broker=%d reason=%s\n", cr.keys[(size_t)p].first.c_str(), cr.keys[(size_t)p].second, cl.brokers[row[j]],
                                 !outside ? "row_holds_every_live_broker" : !ok ? "rack_rule" : "max_rounds");
                }
            }
        }
        if (banded && stats[12] > 0)   // the band never forced anything: a warning, status 0
            std::fprintf(stderr, "kao-disk: warning: %lld brokers hold a replica count outside the band %d:%d\n", (long long)stats[12], band_lo, band_hi);
        const std::string text = changed_rows_text(cr, rows, cl.brokers);
        std::ofstream f(out_path);
        f << text;
        f.close();
        if (!f) throw std::runtime_error("cannot write " + out_path);
        kao_shutdown();
        return n_left > 0 ? 3 : 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "kao-disk: %s\n", e.what());
        return 1;
    }
}
