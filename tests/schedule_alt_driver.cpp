// schedule_alt_driver.cpp -- the step schedule (csrc/host_schedule.h) as a stand-alone program with CallShape::alternate_stores,
// for tests/test_schedule_alt_cpu.py: tests/schedule_driver.cpp's script format with one more flag and one more op.
// stdin: one script per line, "<scheme> <light_inner_steps> <readonly_c> <alternate_stores> <op> <op> ...", run on a freshly
// created schedule.  Ops:
//   r refresh | i invalidate | sN N plain steps | eN N steps under a held field | pN ... under per-step fields | hN ... under a held
//   action | aN ... under per-step actions | fN N steps under the feedback law | g the next pic_step_stage | c the ring take of a
//   copy into a handle without a cached deposit | kX pic_set_integrator(X) | oB pic_set_readonly_c(B) | tB pic_set_alternate_stores(B)
//   [ remember the schedule as it stands | ] return to the one remembered last (a test walks a tree of scripts without replaying each
//   prefix); both print themselves
// An op the entry points refuse while a staged step is open prints "O <op> refused" and changes nothing.
// stdout, per script: "B <script>"; per op "O <op>", one "L ..." per launch (the Launch's fields in declaration order; turn before
// hand_on; last, the rows retired since the line before, or "-") and one "S ..." with the state left behind (ride / pend: what the
// call left riding or pending; ret as for a launch).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host_plan.h"
#include "host_schedule.h"

// the rows that have joined the ring's dirty list since the last call (those `l` is about to clear included)
static bool was[RING];      // the dirty list at the line before
static void print_retired(const Ring& ring, const Launch* l) {
  bool now[RING] = {};
  for (int k = 0; k < ring.ndirty; ++k) now[ring.dirty[k]] = true;
  const char* sep = " ";
  for (int s = 0; s < RING; ++s) {
    if ((now[s] || (l && (l->clear[0] == s || l->clear[1] == s))) && !was[s]) { std::printf("%s%d", sep, s); sep = ","; }
    was[s] = now[s];
  }
  std::printf("%s\n", sep[0] == ' ' ? " -" : "");
}

static void print_launch(const Ring& ring, const Launch& l) {
  std::printf("L %d %a %a %a %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", l.stage, l.c_prev, l.c_cur, l.d_cur, l.in, l.fill[0],
              l.fill[1], l.unclean, l.post, l.clear[0], l.clear[1], l.reverse, l.ctl, l.ext_out, l.turn, (int)l.hand_on, l.step,
              l.post_step, (int)l.retire, (int)l.feedback);
  print_retired(ring, &l);
}

static void print_state(const Schedule& S, const CallLocals& L) {
  std::printf("S q=%d st=%d mid=%d par=%d turn=%d ride=%d pend=%d clean=", S.q_slot, S.stage_slot, S.mid_stage, S.sweep_parity,
              S.ext_turn, L.post, (int)L.refresh_pending);
  for (int k = 0; k < S.ring.nclean; ++k) std::printf("%s%d", k ? "," : "", S.ring.clean[k]);
  std::printf(" dirty=");
  for (int k = 0; k < S.ring.ndirty; ++k) std::printf("%s%d", k ? "," : "", S.ring.dirty[k]);
  print_retired(S.ring, nullptr);
}

int main() {
  double cs[4], ds[4];
  yoshida_coefficients(cs, ds);
  static char line[1 << 20];
  while (std::fgets(line, sizeof line, stdin)) {
    line[std::strcspn(line, "\n")] = 0;
    std::printf("B %.100s\n", line);
    Schedule S;
    std::memset(was, 0, sizeof was);
    auto emit = [&S](const Launch& l) { print_launch(S.ring, l); };
    CallShape base;
    base.cs = cs; base.ds = ds;
    struct Saved { Schedule S; CallShape base; bool was[RING]; } saved[16];
    int nsaved = 0;
    int field = 0;
    for (char* tok = std::strtok(line, " "); tok; tok = std::strtok(nullptr, " "), ++field) {
      const int n = tok[1] ? std::atoi(tok + 1) : 0;
      if (field == 0) { base.scheme = std::atoi(tok); continue; }
      if (field == 1) { base.light_inner_steps = std::atoi(tok) != 0; continue; }
      if (field == 2) { base.readonly_c = std::atoi(tok) != 0; continue; }
      if (field == 3) { base.alternate_stores = std::atoi(tok) != 0; continue; }
      const char op = tok[0];
      if (op == '[' || op == ']') {
        std::printf("%c\n", op);
        if (op == '[' && nsaved < 16) {
          saved[nsaved].S = S; saved[nsaved].base = base;
          std::memcpy(saved[nsaved++].was, was, sizeof was);
        } else if (op == ']' && nsaved > 0) {
          S = saved[--nsaved].S; base = saved[nsaved].base;
          std::memcpy(was, saved[nsaved].was, sizeof was);
        } else {
          std::fprintf(stderr, "schedule_alt_driver: unbalanced %c\n", op);
          return 2;
        }
        continue;
      }
      if (S.mid_stage && std::strchr("sephafck", op)) {      // (the two mode setters are not refused: they change no state)
        std::printf("O %s refused\n", tok);
        continue;
      }
      std::printf("O %s\n", tok);
      CallLocals L;
      CallShape p = base;
      switch (op) {
        case 'r': plan_refresh(S, base.scheme, emit); break;
        case 'i': plan_drop(S); break;
        case 'g': plan_stage(S, base, S.mid_stage + 1, emit); break;
        case 'c':
          if (S.q_slot < 0) {
            bool unclean = false;
            S.q_slot = S.ring.take(&unclean);
            if (unclean) std::printf("L unclean take\n");
          }
          break;
        case 'k':
          if (n != base.scheme) {
            plan_drop(S);
            base.scheme = n;
          }
          break;
        case 'o': base.readonly_c = n != 0; break;
        case 't': base.alternate_stores = n != 0; break;
        case 's': case 'e': case 'p': case 'h': case 'a': case 'f':
          p.feedback = op == 'f';
          p.action = op == 'h' || op == 'a';
          p.per_step_field = op == 'p';
          p.per_step_action = op == 'a';
          L = plan_call(S, p, n, emit);
          break;
        default:
          std::fprintf(stderr, "schedule_alt_driver: unknown op: %s\n", tok);
          return 2;
      }
      print_state(S, L);
    }
  }
  return 0;
}
