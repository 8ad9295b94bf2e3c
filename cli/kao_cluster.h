// kao_cluster.h -- what kao-leaders and kao-failover share: the --broker-list / --racks arguments as kao-cli reads them, and the
// quoting of a topic name in the reassignment documents they write.
#pragma once
#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

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
