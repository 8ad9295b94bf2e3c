// kao_sizes.h -- what kao-waves, kao-leaders, kao-failover, kao-disk and kao-logdirs share: partition sizes read from `kafka-log-dirs --describe` output or a
// sizes document (kao-waves --sizes, kao-leaders --sizes, kao-failover --sizes), the same output WITH its directories (kao-logdirs
// --log-dirs), and the traffic document of kao-leaders --traffic and kao-failover --traffic; byte counts with a K / M / G / T suffix
// (kao-waves --max-bytes-per-broker, kao-disk --min-gain).
#pragma once
#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "kao_json.h"

using Key = std::pair<std::string, int>;   // (topic, partition)

constexpr uint64_t kMaxSize = uint64_t(1) << 53;   // JSON numbers are doubles here: exact up to 2^53, larger sizes are rejected

// N, or N with a K / M / G / T suffix (powers of 1024), below 2^64; false when it is not one
inline bool parse_bytes(const std::string &text, uint64_t &out) {
    std::string t = text;
    uint64_t mult = 1;
    if (!t.empty()) {
        const char c = (char)std::toupper((unsigned char)t.back());
        const char *units = "KMGT", *u = std::strchr(units, c);
        if (c && u) {
            for (int i = 0; i <= u - units; ++i) mult *= 1024;
            t.pop_back();
        }
    }
    if (t.empty() || t.size() > 20 || t.find_first_not_of("0123456789") != std::string::npos) return false;
    errno = 0;
    const unsigned long long v = std::strtoull(t.c_str(), nullptr, 10);
    if (errno == ERANGE || (mult > 1 && v > UINT64_MAX / mult)) return false;
    out = (uint64_t)v * mult;
    return true;
}

// --capacities of kao-disk and kao-waves: id:bytes,id:bytes or a JSON file {"<brokerId>": bytes}, a value a number or a string, each N
// or N with K/M/G/T
inline std::map<int, uint64_t> read_broker_capacities(const std::string &arg) {
    std::map<int, uint64_t> out;
    auto put = [&](const std::string &id, const std::string &text) {
        uint64_t v = 0;
        if (id.empty() || id.find_first_not_of("0123456789") != std::string::npos || !parse_bytes(text, v))
            throw std::runtime_error("capacity of broker " + id + ": not a byte count: " + text);
        out[std::atoi(id.c_str())] = v;
    };
    if (arg.find(':') != std::string::npos && arg.find('{') == std::string::npos && (arg.size() < 5 || arg.compare(arg.size() - 5, 5, ".json") != 0)) {
        std::istringstream in(arg);
        std::string t;
        while (std::getline(in, t, ',')) {
            t.erase(std::remove_if(t.begin(), t.end(), [](unsigned char c) { return std::isspace(c) != 0; }), t.end());
            if (t.empty()) continue;
            const size_t colon = t.find(':');
            if (colon == std::string::npos || t.find(':', colon + 1) != std::string::npos) throw std::runtime_error("bad --capacities entry " + t);
            put(t.substr(0, colon), t.substr(colon + 1));
        }
    } else {
        const std::string txt = slurp(arg);
        const JValue doc = JParser(txt).parse();
        if (doc.kind != JValue::Obj) throw std::runtime_error("capacities file must be a JSON object {\"<brokerId>\": bytes}");
        for (auto &kv : doc.obj) {
            if (kv.second.kind != JValue::Num && kv.second.kind != JValue::Str) throw std::runtime_error("capacity of broker " + kv.first + ": not a byte count");
            put(kv.first, kv.second.kind == JValue::Num ? kv.second.raw : kv.second.str);
        }
    }
    return out;
}

inline uint64_t size_value(const JValue *v, const std::string &what) {
    uint64_t x = 0;
    if (!v || v->kind != JValue::Num || v->raw.empty() || v->raw.size() > 16 || v->raw.find_first_not_of("0123456789") != std::string::npos ||
        (x = std::strtoull(v->raw.c_str(), nullptr, 10)) > kMaxSize)
        throw std::runtime_error("sizes: " + what + ": size must be an integer 0..2^53");
    return x;
}

// partition sizes, from `kafka-log-dirs --describe` output (the largest non-future replica; names split at the last '-') or from a
// {"partitions":[{"topic","partition","size"}]} document
inline std::map<Key, uint64_t> load_sizes(const std::string &path) {
    const std::string txt = slurp(path);
    JValue doc;
    try {
        doc = JParser(txt).parse();
    } catch (const std::runtime_error &) {   // kafka-log-dirs prints status lines before its JSON line
        std::istringstream in(txt);
        std::string line;
        bool found = false;
        while (!found && std::getline(in, line)) {
            const size_t b = line.find_first_not_of(" \t\r");
            if (b != std::string::npos && line[b] == '{') { doc = JParser(line).parse(); found = true; }
        }
        if (!found) throw std::runtime_error("sizes: no JSON document found");
    }
    std::map<Key, uint64_t> out;
    if (const JValue *brokers = doc.get("brokers")) {
        for (auto &br : brokers->arr) {
            const JValue *dirs = br.get("logDirs");
            if (!dirs) continue;
            for (auto &d : dirs->arr) {
                const JValue *parts = d.get("partitions");
                if (!parts) continue;
                for (auto &e : parts->arr) {
                    const JValue *fut = e.get("isFuture"), *name = e.get("partition");
                    if (fut && fut->kind == JValue::Bool && fut->b) continue;
                    if (!name || name->kind != JValue::Str) throw std::runtime_error("sizes: log-dir entry without a partition name");
                    const size_t dash = name->str.rfind('-');
                    const std::string idx = dash == std::string::npos ? "" : name->str.substr(dash + 1);
                    if (dash == std::string::npos || dash == 0 || idx.empty() || idx.size() > 9 || idx.find_first_not_of("0123456789") != std::string::npos)
                        throw std::runtime_error("sizes: partition name '" + name->str + "' is not <topic>-<partition>");
                    const Key k{name->str.substr(0, dash), std::atoi(idx.c_str())};
                    const uint64_t v = size_value(e.get("size"), name->str);
                    auto it = out.find(k);
                    if (it == out.end()) out[k] = v;
                    else it->second = std::max(it->second, v);
                }
            }
        }
    } else if (const JValue *parts = doc.get("partitions")) {
        for (auto &e : parts->arr) {
            const JValue *t = e.get("topic"), *p = e.get("partition");
            if (!t || !p) throw std::runtime_error("sizes: partition entry needs topic/partition/size");
            const Key k{t->str, (int)p->num};
            const std::string what = k.first + "-" + std::to_string(k.second);
            if (out.count(k)) throw std::runtime_error("sizes: partition " + what + " listed twice");
            out[k] = size_value(e.get("size"), what);
        }
    } else {
        throw std::runtime_error("sizes: expected a \"brokers\" (kafka-log-dirs) or \"partitions\" document");
    }
    return out;
}

// `kafka-log-dirs --describe` output with what load_sizes folds away: per broker its log dirs in the order of the document, each with
// its name, whether its "error" is non-null, its entries (partition names split at the last '-'; sizes 0..2^53; isFuture), and the
// totalBytes / usableBytes of its volume where the document has them (Kafka >= 3.3; absent or null: has_* stays false).
struct LogDirEntry {
    Key key;
    uint64_t size = 0;
    bool future = false;
};
struct LogDir {
    std::string name;
    bool failed = false;
    std::vector<LogDirEntry> entries;
    bool has_total = false, has_usable = false;
    uint64_t total_bytes = 0, usable_bytes = 0;
};
// totalBytes / usableBytes of a log dir: false when absent or null, else an integer 0..2^53 under the rules of a size
inline bool volume_bytes(const JValue *v, const std::string &what, uint64_t &out) {
    if (!v || v->kind == JValue::Null) return false;
    if (v->kind != JValue::Num || v->raw.empty() || v->raw.size() > 16 || v->raw.find_first_not_of("0123456789") != std::string::npos ||
        (out = std::strtoull(v->raw.c_str(), nullptr, 10)) > kMaxSize)
        throw std::runtime_error(what + ": size must be an integer 0..2^53");
    return true;
}
inline std::map<int, std::vector<LogDir>> load_log_dirs(const std::string &path) {
    const std::string txt = slurp(path);
    JValue doc;
    try {
        doc = JParser(txt).parse();
    } catch (const std::runtime_error &) {   // kafka-log-dirs prints status lines before its JSON line
        std::istringstream in(txt);
        std::string line;
        bool found = false;
        while (!found && std::getline(in, line)) {
            const size_t b = line.find_first_not_of(" \t\r");
            if (b != std::string::npos && line[b] == '{') { doc = JParser(line).parse(); found = true; }
        }
        if (!found) throw std::runtime_error("log-dirs: no JSON document found");
    }
    const JValue *brokers = doc.get("brokers");
    if (!brokers || brokers->kind != JValue::Arr) throw std::runtime_error("log-dirs: expected a \"brokers\" (kafka-log-dirs) document");
    std::map<int, std::vector<LogDir>> out;
    for (auto &br : brokers->arr) {
        const JValue *id = br.get("broker");
        if (!id || id->kind != JValue::Num || id->raw.find_first_not_of("-0123456789") != std::string::npos) throw std::runtime_error("log-dirs: broker entry without an integer id");
        const int b = (int)id->num;
        if (out.count(b)) throw std::runtime_error("log-dirs: broker " + std::to_string(b) + " listed twice");
        std::vector<LogDir> &dirs = out[b];
        const JValue *lds = br.get("logDirs");
        if (!lds) continue;
        for (auto &ld : lds->arr) {
            const JValue *name = ld.get("logDir"), *err = ld.get("error"), *parts = ld.get("partitions");
            if (!name || name->kind != JValue::Str) throw std::runtime_error("log-dirs: broker " + std::to_string(b) + ": log dir without a name");
            for (auto &d : dirs)
                if (d.name == name->str) throw std::runtime_error("log-dirs: broker " + std::to_string(b) + ": log dir " + name->str + " listed twice");
            LogDir dir;
            dir.name = name->str;
            dir.failed = err && err->kind != JValue::Null;
            dir.has_total = volume_bytes(ld.get("totalBytes"), "log-dirs: broker " + std::to_string(b) + ": " + name->str + ": totalBytes", dir.total_bytes);
            dir.has_usable = volume_bytes(ld.get("usableBytes"), "log-dirs: broker " + std::to_string(b) + ": " + name->str + ": usableBytes", dir.usable_bytes);
            for (size_t i = 0; parts && i < parts->arr.size(); ++i) {
                const JValue &e = parts->arr[i];
                const JValue *fut = e.get("isFuture"), *pn = e.get("partition"), *v = e.get("size");
                if (!pn || pn->kind != JValue::Str) throw std::runtime_error("log-dirs: log-dir entry without a partition name");
                const size_t dash = pn->str.rfind('-');
                const std::string idx = dash == std::string::npos ? "" : pn->str.substr(dash + 1);
                if (dash == std::string::npos || dash == 0 || idx.empty() || idx.size() > 9 || idx.find_first_not_of("0123456789") != std::string::npos)
                    throw std::runtime_error("log-dirs: partition name '" + pn->str + "' is not <topic>-<partition>");
                LogDirEntry en;
                en.key = Key{pn->str.substr(0, dash), std::atoi(idx.c_str())};
                if (!v || v->kind != JValue::Num || v->raw.empty() || v->raw.size() > 16 || v->raw.find_first_not_of("0123456789") != std::string::npos ||
                    (en.size = std::strtoull(v->raw.c_str(), nullptr, 10)) > kMaxSize)
                    throw std::runtime_error("log-dirs: " + pn->str + ": size must be an integer 0..2^53");
                en.future = fut && fut->kind == JValue::Bool && fut->b;
                dir.entries.push_back(en);
            }
            dirs.push_back(dir);
        }
    }
    return out;
}

// partition weights from {"version":1,"partitions":[{"topic":..,"partition":..,"weight":N}]}: N an integer 0..2^53, no partition twice
inline std::map<Key, uint64_t> load_traffic(const std::string &path) {
    const std::string txt = slurp(path);
    const JValue doc = JParser(txt).parse();
    const JValue *parts = doc.get("partitions");
    if (!parts || parts->kind != JValue::Arr) throw std::runtime_error("traffic: missing \"partitions\" array");
    std::map<Key, uint64_t> out;
    for (auto &e : parts->arr) {
        const JValue *t = e.get("topic"), *p = e.get("partition"), *v = e.get("weight");
        if (!t || !p) throw std::runtime_error("traffic: partition entry needs topic/partition/weight");
        const Key k{t->str, (int)p->num};
        const std::string what = k.first + "-" + std::to_string(k.second);
        if (out.count(k)) throw std::runtime_error("traffic: partition " + what + " listed twice");
        uint64_t x = 0;
        if (!v || v->kind != JValue::Num || v->raw.empty() || v->raw.size() > 16 || v->raw.find_first_not_of("0123456789") != std::string::npos ||
            (x = std::strtoull(v->raw.c_str(), nullptr, 10)) > kMaxSize)
            throw std::runtime_error("traffic: " + what + ": weight must be an integer 0..2^53");
        out[k] = x;
    }
    return out;
}
