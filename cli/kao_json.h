// kao_json.h -- the minimal JSON reader of the command-line tools (objects, arrays, strings, numbers, true/false/null) and a
// whole-file reader.  Header-only; each tool includes it once.
#pragma once
#include <cctype>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace {

struct JValue {
    enum Kind { Null, Bool, Num, Str, Arr, Obj } kind = Null;
    double num = 0;
    bool b = false;
    std::string str;
    std::string raw;   // a number's source text
    std::vector<JValue> arr;
    std::vector<std::pair<std::string, JValue>> obj;
    const JValue *get(const std::string &k) const {
        for (auto &kv : obj) if (kv.first == k) return &kv.second;
        return nullptr;
    }
};

struct JParser {
    const std::string &s;
    size_t i = 0;
    explicit JParser(const std::string &src) : s(src) {}
    [[noreturn]] void bad(const char *what) { throw std::runtime_error(std::string("JSON: ") + what + " at offset " + std::to_string(i)); }
    void ws() { while (i < s.size() && std::isspace((unsigned char)s[i])) ++i; }
    JValue parse() { JValue v = value(); ws(); if (i != s.size()) bad("trailing characters"); return v; }
    JValue value() {
        ws();
        if (i >= s.size()) bad("unexpected end");
        char c = s[i];
        JValue v;
        if (c == '{') {
            v.kind = JValue::Obj; ++i; ws();
            if (i < s.size() && s[i] == '}') { ++i; return v; }
            for (;;) {
                ws(); JValue k = value();
                if (k.kind != JValue::Str) bad("object key must be a string");
                ws(); if (i >= s.size() || s[i] != ':') bad("expected ':'"); ++i;
                v.obj.emplace_back(k.str, value());
                ws(); if (i < s.size() && s[i] == ',') { ++i; continue; }
                if (i < s.size() && s[i] == '}') { ++i; return v; }
                bad("expected ',' or '}'");
            }
        }
        if (c == '[') {
            v.kind = JValue::Arr; ++i; ws();
            if (i < s.size() && s[i] == ']') { ++i; return v; }
            for (;;) {
                v.arr.push_back(value());
                ws(); if (i < s.size() && s[i] == ',') { ++i; continue; }
                if (i < s.size() && s[i] == ']') { ++i; return v; }
                bad("expected ',' or ']'");
            }
        }
        if (c == '"') {
            v.kind = JValue::Str; ++i;
            while (i < s.size() && s[i] != '"') {
                if (s[i] == '\\' && i + 1 < s.size()) { ++i; char e = s[i]; v.str += (e == 'n' ? '\n' : e == 't' ? '\t' : e); }
                else v.str += s[i];
                ++i;
            }
            if (i >= s.size()) bad("unterminated string");
            ++i; return v;
        }
        if (c == '-' || std::isdigit((unsigned char)c)) {
            size_t j = i; if (s[j] == '-') ++j;
            while (j < s.size() && (std::isdigit((unsigned char)s[j]) || s[j] == '.' || s[j] == 'e' || s[j] == 'E' || s[j] == '+' || s[j] == '-')) ++j;
            v.kind = JValue::Num; v.raw = s.substr(i, j - i); v.num = std::strtod(v.raw.c_str(), nullptr); i = j; return v;
        }
        if (s.compare(i, 4, "true") == 0) { v.kind = JValue::Bool; v.b = true; i += 4; return v; }
        if (s.compare(i, 5, "false") == 0) { v.kind = JValue::Bool; i += 5; return v; }
        if (s.compare(i, 4, "null") == 0) { i += 4; return v; }
        bad("unexpected character");
    }
};

std::string slurp(const std::string &path) {
    if (path == "-") { std::stringstream ss; ss << std::cin.rdbuf(); return ss.str(); }
    std::ifstream f(path);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::stringstream ss; ss << f.rdbuf(); return ss.str();
}

}  // namespace
