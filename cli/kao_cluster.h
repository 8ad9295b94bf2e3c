// kao_cluster.h -- what kao-leaders, kao-failover and kao-disk share: the --broker-list / --racks arguments as kao-cli reads them, the rows of
// a reassignment document over that broker index, and the reassignment documents they write.
#pragma once
#include <algorithm>
#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../include/kao.h"
#include "kao_json.h"

inline std::vector<std::string> split(const std::string &s, char sep) {
    std::vector<std::string> out; std::string cur;
    for (char c : s) { if (c == sep) { out.push_back(cur); cur.clear(); } else if (!std::isspace((unsigned char)c)) cur += c; }
    if (!cur.empty() || !s.empty()) out.push_back(cur);
    return out;
}

inline std::string quoted(const std::string &s) {
    std::string o = "\"";
    for (char c : s) {
        if (c == '"' || c == '\\') o += '\\';
        o += c;
    }
    return o + "\"";
}

// The cluster of --broker-list (dense index = position in the list) and --racks (a JSON file {"<brokerId>": "<rack>"} or
// id:rack,id:rack); racks are indexed in the order of their names.
struct Cluster {
    std::vector<int> brokers;              // dense index -> broker id
    std::map<int, int> dense;              // broker id -> dense index
    std::vector<std::string> rack_names;   // rack index -> name
    std::vector<uint8_t> rack_of;          // [brokers] rack index
};

inline Cluster read_cluster(const std::string &brokers_csv, const std::string &racks_arg) {
    Cluster c;
    for (auto &t : split(brokers_csv, ',')) if (!t.empty()) c.brokers.push_back(std::atoi(t.c_str()));
    if (c.brokers.empty()) throw std::runtime_error("empty broker list");
    for (size_t i = 0; i < c.brokers.size(); ++i) if (!c.dense.emplace(c.brokers[i], (int)i).second) throw std::runtime_error("duplicate id in broker list");
    std::map<int, std::string> rack_name;
    if (racks_arg.find(':') != std::string::npos && racks_arg.find('{') == std::string::npos) {
        for (auto &t : split(racks_arg, ',')) { auto kv = split(t, ':'); if (kv.size() != 2) throw std::runtime_error("bad --racks entry " + t); rack_name[std::atoi(kv[0].c_str())] = kv[1]; }
    } else {
        std::string txt = slurp(racks_arg);
        JValue doc = JParser(txt).parse();
        if (doc.kind != JValue::Obj) throw std::runtime_error("racks file must be a JSON object {\"<brokerId>\": \"<rack>\"}");
        for (auto &kv : doc.obj) rack_name[std::atoi(kv.first.c_str())] = kv.second.kind == JValue::Str ? kv.second.str : std::to_string((long long)kv.second.num);
    }
    std::set<std::string> names;
    for (int b : c.brokers) { auto it = rack_name.find(b); if (it == rack_name.end()) throw std::runtime_error("no rack given for broker " + std::to_string(b)); names.insert(it->second); }
    std::map<std::string, int> rack_idx;
    for (auto &n : names) { rack_idx[n] = (int)c.rack_names.size(); c.rack_names.push_back(n); }
    for (int b : c.brokers) c.rack_of.push_back((uint8_t)rack_idx[rack_name[b]]);
    return c;
}

// The rows of a reassignment document over the cluster's broker index: the partitions of all topics ordered by (topic, partition),
// `width` = the longest replica list, shorter rows padded with KAO_NONE.  A partition without a replica or with a replica outside
// the broker list is an error.
struct ClusterRows {
    std::vector<std::pair<std::string, int>> keys;   // (topic, partition) per row
    std::vector<uint16_t> rows;                      // [max(keys.size(), 1) * width]
    int width = 1;
};

inline ClusterRows read_rows(const std::string &path, const Cluster &cl) {
    std::string cur_txt = slurp(path);
    JValue doc = JParser(cur_txt).parse();
    const JValue *parts = doc.get("partitions");
    if (!parts || parts->kind != JValue::Arr) throw std::runtime_error("missing \"partitions\" array");
    std::map<std::pair<std::string, int>, std::vector<int>> by_key;
    for (auto &e : parts->arr) {
        const JValue *t = e.get("topic"), *p = e.get("partition"), *r = e.get("replicas");
        if (!t || !p || !r || r->kind != JValue::Arr) throw std::runtime_error("partition entry needs topic/partition/replicas");
        std::vector<int> reps; for (auto &x : r->arr) reps.push_back((int)x.num);
        by_key[{t->str, (int)p->num}] = reps;
    }
    ClusterRows out;
    size_t width = 1;
    for (auto &kv : by_key) width = std::max(width, kv.second.size());
    out.width = (int)width;
    out.rows.assign(std::max(by_key.size(), (size_t)1) * width, (uint16_t)KAO_NONE);
    for (auto &kv : by_key) {
        const std::string name = kv.first.first + "-" + std::to_string(kv.first.second);
        if (kv.second.empty()) throw std::runtime_error("partition " + name + " has no replica");
        for (size_t j = 0; j < kv.second.size(); ++j) {
            auto it = cl.dense.find(kv.second[j]);
            if (it == cl.dense.end()) throw std::runtime_error("partition " + name + " has a replica outside --broker-list (broker " + std::to_string(kv.second[j]) + ")");
            out.rows[out.keys.size() * width + j] = (uint16_t)it->second;
        }
        out.keys.push_back(kv.first);
    }
    return out;
}

// The reassignment document of the rows that differ from `cur`, as broker ids.
inline std::string changed_rows_text(const ClusterRows &cur, const std::vector<uint16_t> &rows, const std::vector<int> &brokers) {
    const int P = (int)cur.keys.size(), W = cur.width;
    int n_out = 0;
    std::string body;
    for (int p = 0; p < P; ++p) {
        if (std::equal(rows.begin() + (size_t)p * W, rows.begin() + (size_t)(p + 1) * W, cur.rows.begin() + (size_t)p * W)) continue;
        body += (n_out++ ? ",\n" : "\n");
        body += "    {\"topic\":" + quoted(cur.keys[(size_t)p].first) + ",\"partition\":" + std::to_string(cur.keys[(size_t)p].second) + ",\"replicas\":[";
        for (int k = 0; k < W && rows[(size_t)p * W + k] != KAO_NONE; ++k) body += (k ? "," : "") + std::to_string(brokers[rows[(size_t)p * W + k]]);
        body += "]}";
    }
    return "{\"version\":1,\"partitions\":[" + body + "\n]}\n";
}
