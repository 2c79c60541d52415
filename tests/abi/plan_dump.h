// What the dump programs of the plan headers share: a request line as a keyword and the words behind it, read as integers or
// doubles; the recordings' counts as rec_start; the answer of a check.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "plan_support.h"

namespace plan_dump {

struct Request {
    std::string what;              // the keyword (empty for an empty line: no dump knows it)
    std::vector<std::string> a;    // the words behind it
    explicit Request(const std::string& line) {
        std::istringstream in(line);
        in >> what;
        for (std::string x; in >> x;) a.push_back(x);
    }
    long long I(size_t k) const { return std::strtoll(a.at(k).c_str(), nullptr, 10); }
    double D(size_t k) const { return std::strtod(a.at(k).c_str(), nullptr); }      // (reads "nan" and "inf" too)
    // rec_start of the request: the words themselves for `start`, else the running sum of the counts behind the first `lead`.
    std::vector<int64_t> rec_start(size_t lead = 0) const {
        std::vector<int64_t> rs;
        if (what != "start") rs.push_back(0);
        for (size_t k = what == "start" ? 0 : lead; k < a.size(); ++k) rs.push_back(what == "start" ? I(k) : rs.back() + I(k));
        return rs;
    }
};

// ok | refused <message>, or toolarge <message> where the check says that the refusal is one of size
inline void answer(int bad, const xvec::Refusal& why, bool too_large = false) {
    if (bad) std::printf("%s %s\n", too_large ? "toolarge" : "refused", why.text); else std::printf("ok\n");
}

}  // namespace plan_dump
