// load_probe -- what a load checks and installs (csrc/faasbal_load.h) from the command line, no GPU.
//
// Reads one request per line on stdin and answers each with one line of key=value words.
//   conditions        the names of LoadRefusal, in order
//   load k=v ...      load_check, and load_image if it accepts.  The kind's facts: deque sharded
//                     inflight win W_cap W_global Wq_cap log_cap.  The counts: base n qlen llen
//                     head.  The arrays: reg free hb epoch queue log seq, each "-" (a null
//                     pointer), "." (empty, not null) or values joined by commas.
//                     Answer: rc=..., then (rc = 0) the image's arrays in the same notation
//                     ("." where the kind has none) and maxc=..., then msg=... to the line's end.
// Built by tests/test_load_host.py; it makes no HIP runtime call.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "faasbal_load.h"

using namespace fb;

namespace {

// an array argument: null, or a pointer that is never null (one spare element behind the values)
template <typename T>
struct Arr {
    std::vector<T> v;
    bool null = true;
    const T *ptr() const { return null ? nullptr : v.data(); }
};
template <typename T>
Arr<T> parse(const std::map<std::string, std::string> &kv, const char *key) {
    Arr<T> a;
    const auto it = kv.find(key);
    if (it == kv.end() || it->second == "-") return a;
    a.null = false;
    if (it->second != ".") {
        std::istringstream ss(it->second);
        std::string w;
        while (std::getline(ss, w, ',')) a.v.push_back((T)std::strtod(w.c_str(), nullptr));  // (integers: exact)
    }
    a.v.push_back(T());
    return a;
}

template <typename V, typename F>
void put(const char *key, const V &v, F one) {
    std::printf(" %s=", key);
    if (v.empty()) std::printf(".");
    for (size_t i = 0; i < v.size(); ++i) {
        if (i) std::printf(",");
        one(v[i]);
    }
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ss(line);
        std::string cmd, w;
        ss >> cmd;
        if (cmd == "conditions") {
            for (int i = 0; i < (int)LoadRefusal::count_; ++i) std::printf("%s%s", i ? " " : "", kLoadRefusals[i].name);
            std::printf("\n");
            continue;
        }
        if (cmd != "load") {
            std::printf("error=unknown request\n");
            continue;
        }
        std::map<std::string, std::string> kv;
        while (ss >> w) kv[w.substr(0, w.find('='))] = w.substr(w.find('=') + 1);
        const auto num = [&](const char *key) { return std::strtoll(kv[key].c_str(), nullptr, 10); };
        LoadKind k;
        k.deque = num("deque") != 0;
        k.sharded = num("sharded") != 0;
        k.inflight = num("inflight") != 0;
        k.win_cap = num("win") != 0;
        k.W_cap = (int32_t)num("W_cap");
        k.W_global = (int32_t)num("W_global");
        k.Wq_cap = (int32_t)num("Wq_cap");
        k.log_cap = num("log_cap");
        const Arr<uint8_t> reg = parse<uint8_t>(kv, "reg");
        const Arr<int32_t> fr = parse<int32_t>(kv, "free"), queue = parse<int32_t>(kv, "queue"), log = parse<int32_t>(kv, "log");
        const Arr<double> hb = parse<double>(kv, "hb");
        const Arr<uint32_t> epoch = parse<uint32_t>(kv, "epoch"), seq = parse<uint32_t>(kv, "seq");
        const LoadIn in{(int32_t)num("base"), (int32_t)num("n"), reg.ptr(), fr.ptr(), hb.ptr(), epoch.ptr(), queue.ptr(),
                        num("qlen"), log.ptr(), seq.ptr(), num("llen"), num("head")};
        std::string msg;
        const int rc = load_check(k, in, msg);
        std::printf("rc=%d", rc);
        if (rc == FB_OK) {
            const LoadImage m = load_image(k, in);
            const auto i32 = [](int32_t x) { std::printf("%d", x); };
            const auto u32 = [](uint32_t x) { std::printf("%u", x); };
            const auto f64 = [](double x) { std::printf("%.17g", x); };
            std::vector<int32_t> fq_free, fq_inq;
            for (const LoadPair &p : m.fq) {
                fq_free.push_back(p.free);
                fq_inq.push_back(p.inq);
            }
            put("reg", m.reg, [](uint8_t x) { std::printf("%d", (int)x); });
            put("hb", m.hb, f64);
            put("epoch", m.epoch, u32);
            put("free", fq_free, i32);
            put("inq", fq_inq, i32);
            put("pos", m.pos, i32);
            put("qfree", m.qfree, i32);
            put("qhb", m.qhb, f64);
            put("tokcnt", m.tokcnt, i32);
            put("qrank", m.qrank, u32);
            put("log", m.log, i32);
            put("bud", m.bud, i32);
            std::printf(" maxc=%d", m.maxc);
        }
        std::printf(" msg=%s\n", msg.c_str());
    }
    return 0;
}
