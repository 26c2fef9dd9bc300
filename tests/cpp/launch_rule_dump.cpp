// The launch rule (csrc/gtop_launch_rule.cpp) over every switch point, as text: tests/test_launch_rule.py compares the
// output with tests/golden/launch_rule.txt.  Plain C++, no HIP.
//   launch_rule_dump          the table: one code character per plan (legend in the first lines), '.' = refused;
//                             one line per run of segment counts m with the same codes over the batch sizes
//   launch_rule_dump --check  one line per accepted plan that breaks what the rule's callers rely on (none: no output)
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "gtop_launch_rule.h"

namespace {

const int kB[] = {1,    512,  513,  1023,  1024,  1025,  2047,  2048,  3071,  3072,  4095,
                  4096, 8191, 8192, 12288, 16384, 32767, 32768, 65535, 65536, 131072};
const int kPins[] = {0, 3, 6, 10, 30, 5 /* illegal */};
const size_t kElems[] = {8, 4};

std::vector<int> segment_counts() {
  std::vector<int> m;
  for (int i = 1; i <= 70; ++i) m.push_back(i);
  for (int i : {118, 119, 227, 228}) m.push_back(i);
  return m;
}

using Plan = std::tuple<int, int, int, int>;   // spl, nt, is_long, nw
struct Case {
  bool moving;
  int fo, pin, m, B;
  size_t elem;
  bool ok;
  GtopEvalPlan p;
};

std::vector<Case> all_cases() {
  std::vector<Case> out;
  const std::vector<int> ms = segment_counts();
  for (int moving = 0; moving < 2; ++moving)
    for (int fo = 0; fo < 2; ++fo)
      for (size_t elem : kElems) {
        if (moving && elem != 8) continue;   // (the moving-term bodies are fp64)
        for (int pin : kPins)
          for (int m : ms)
            for (int B : kB) {
              Case c{moving != 0, fo, pin, m, B, elem, false, GtopEvalPlan{}};
              c.ok = moving ? gtop_eval_plan_moving(B, m, pin, fo != 0, &c.p) : gtop_eval_plan(B, m, elem, pin, fo != 0, &c.p);
              out.push_back(c);
            }
      }
  return out;
}

int check(const std::vector<Case> &cases) {
  int bad = 0;
  for (const Case &c : cases) {
    if (!c.ok) continue;
    const GtopEvalPlan &p = c.p;
    char why[128] = "";
    // (the optimizer's state and tile are fp64 whatever precision its evaluations run in)
    const size_t lds = gtop_wave_lds_bytes(p, c.m, c.fo ? sizeof(double) : c.elem, c.fo != 0);
    if (lds > 160u * 1024u) snprintf(why, sizeof why, "%zu bytes of LDS", lds);
    const int slots = p.nw * (64 / (kSamples / p.spl));
    if (!p.is_long && p.nt * c.m > slots) snprintf(why, sizeof why, "%d x %d segments in %d slots", p.nt, c.m, slots);
    if (c.moving && (p.nw != 1 || (p.spl != 3 && p.spl != 6))) snprintf(why, sizeof why, "no moving-term body");
    if (why[0]) {
      printf("%s fo=%d elem=%zu pin=%d m=%d B=%d: spl=%d nt=%d long=%d nw=%d: %s\n", c.moving ? "moving" : "plan", c.fo,
             c.elem, c.pin, c.m, c.B, p.spl, p.nt, (int)p.is_long, p.nw, why);
      ++bad;
    }
  }
  return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
  const std::vector<Case> cases = all_cases();
  if (argc > 1 && !strcmp(argv[1], "--check")) return check(cases);
  std::map<Plan, char> code;
  for (const Case &c : cases)
    if (c.ok) code[Plan(c.p.spl, c.p.nt, c.p.is_long, c.p.nw)] = 0;
  const char *alphabet = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz";
  size_t k = 0;
  for (auto &e : code) {
    if (k >= strlen(alphabet)) return 2;
    e.second = alphabet[k++];
  }
  printf("# B:");
  for (int B : kB) printf(" %d", B);
  printf("\n# one character per B; . = refused");
  for (const auto &e : code)
    printf("\n# %c = spl %d nt %d long %d nw %d", e.second, std::get<0>(e.first), std::get<1>(e.first), std::get<2>(e.first),
           std::get<3>(e.first));
  printf("\n");
  const size_t nB = sizeof kB / sizeof kB[0];
  std::string run;
  int m_lo = 0, m_hi = 0;
  auto flush = [&]() {
    if (!run.empty() && m_lo == m_hi) printf("%d %s\n", m_lo, run.c_str());
    else if (!run.empty()) printf("%d-%d %s\n", m_lo, m_hi, run.c_str());
    run.clear();
  };
  for (size_t i = 0; i < cases.size(); i += nB) {
    const Case &c0 = cases[i];
    if (i == 0 || c0.moving != cases[i - nB].moving || c0.fo != cases[i - nB].fo || c0.elem != cases[i - nB].elem ||
        c0.pin != cases[i - nB].pin) {
      flush();
      printf("%s for_optimizer=%d elem=%zu pin=%d\n", c0.moving ? "moving" : "plan", c0.fo, c0.elem, c0.pin);
    }
    std::string s;
    for (size_t j = 0; j < nB; ++j) {
      const Case &c = cases[i + j];
      s += c.ok ? code[Plan(c.p.spl, c.p.nt, c.p.is_long, c.p.nw)] : '.';
    }
    if (s == run && c0.m == m_hi + 1) {
      m_hi = c0.m;
    } else {
      flush();
      run = s;
      m_lo = m_hi = c0.m;
    }
  }
  flush();
  return 0;
}
