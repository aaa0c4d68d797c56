// Host program around ggrs_amd/csrc/p2p_plan.h (tests/test_p2p_plan.py): reads planner cases from
// stdin, one per line, runs each advance the way ggrs_p2p_advance_frames / p2p_sched_advance loop
// over the plan, and prints every launch in the format of tests/p2p_plan_cases.json.
//   fixed S P mask latency delay maxp cap predictor sparse trace desync dbg(0 none, 1 armed, 2 disarmed) form cus k n1..nk
//   sched S P mask delay maxp cap predictor sparse desync reports trace cus SPLIT CHAINS K k n1..nk
// (SPLIT, CHAINS, K: the values of GGRS_SCHED_SPLIT, GGRS_SCHED_CHAINS and GGRS_SCHED_K, "-" for unset.)
// A second plan of every input must give the same launch ("UNSTABLE" otherwise).
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "p2p_plan.h"

using namespace ggrs;

static std::string show(const P2PLaunch& L, int P, int f0) {
  char b[256], tail[96];
  snprintf(tail, sizeof tail, "grid=%u block=%u lds=%zu f0=%d n=%d", L.grid, L.block, L.lds, f0, L.n);
  const char* name = kP2PKernelNames[(int)L.kernel];
  switch (L.kernel) {
    case P2PKernel::kLockstep: snprintf(b, sizeof b, "%s P=%d %s", name, P, tail); break;
    case P2PKernel::kUnstaged:
    case P2PKernel::kStaged:
      snprintf(b, sizeof b, "%s P=%d staged=%d %s", name, P, L.kernel == P2PKernel::kStaged, tail);
      break;
    case P2PKernel::kFlat:
      snprintf(b, sizeof b, "%s P=%d kLocal=%d plain=%d sparse=%d lds_ring=%d %s", name, P, L.kLocal, L.plain, L.sparse,
               L.lds_ring, tail);
      break;
    case P2PKernel::kCanon:
    case P2PKernel::kCanonSparse: snprintf(b, sizeof b, "%s P=%d kLocal=%d %s", name, P, L.kLocal, tail); break;
    case P2PKernel::kChains:
      snprintf(b, sizeof b, "%s P=%d batch=%d fast=%d spw=%d %s", name, P, L.chain_batch, L.chain_fast, L.spw, tail);
      break;
  }
  return b;
}

static std::string show(const SchedLaunch& L, const SchedPlanIn& in, int c0) {
  char b[320];
  if (L.chains)
    snprintf(b, sizeof b, "sched_chains P=%d pred=%d kLocal=%d feat=%d K=%d B=%d WL=%d TW=%d grid=%u block=%u lds=%zu f0=%d n=%d",
             in.players, in.predictor, L.kLocal, L.feat, L.K, L.B, L.WL, L.TW, L.grid, L.block, L.lds, c0, L.n);
  else
    snprintf(b, sizeof b,
             "sched P=%d sparse=%d pred=%d kLocal=%d split=%d feat=%d K=%d B=%d WL=%d TW=%d nbuf=%d grid=%u block=%u lds=%zu "
             "f0=%d n=%d",
             in.players, in.sparse, in.predictor, L.kLocal, L.split, L.feat, L.K, L.B, L.WL, L.TW, L.nbuf, L.grid, L.block,
             L.lds, c0, L.n);
  return b;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string mode;
    if (!(is >> mode)) continue;
    printf("CASE\n");
    int k = 0, f0 = 0;
    bool failed = false;
    if (mode == "fixed") {
      P2PPlanIn in{};
      int sparse, trace, desync, dbg, form;
      is >> in.sessions >> in.players >> in.local_mask >> in.remote_latency >> in.input_delay >> in.max_prediction >> in.cap >>
          in.predictor >> sparse >> trace >> desync >> dbg >> form >> in.num_cus >> k;
      in.R = in.max_prediction + 1;
      in.sparse = sparse, in.trace = trace, in.desync = desync, in.dbg_armed = dbg == 1, in.dbg_ever = dbg != 0;
      in.form = (P2PForm)form;
      for (int a = 0; a < k && !failed; a++) {
        is >> in.left;
        printf("ADVANCE %d\n", in.left);
        in.f0 = f0, in.row_left = 0;
        while (in.left > 0) {
          P2PLaunch L, again;
          const char *msg = nullptr, *msg2 = nullptr;
          const int rc = p2p_plan_next(in, &L, &msg);
          if (p2p_plan_next(in, &again, &msg2) != rc || (rc == 0 && show(again, in.players, in.f0) != show(L, in.players, in.f0)))
            printf("UNSTABLE\n");
          if (rc) {
            printf("ERROR %d %s\n", rc, msg);
            failed = true;
            break;
          }
          printf("%s\n", show(L, in.players, in.f0).c_str());
          if (L.n < 1 || L.n > in.left) return 2;  // (a plan that does not advance would never end)
          in.f0 += L.n, in.left -= L.n, in.row_left = L.row_left;
        }
        f0 = in.f0;
      }
    } else if (mode == "sched") {
      SchedPlanIn in{};
      int sparse, desync, reports, trace;
      std::string env[3];
      is >> in.sessions >> in.players >> in.local_mask >> in.input_delay >> in.max_prediction >> in.cap >> in.predictor >>
          sparse >> desync >> reports >> trace >> in.num_cus >> env[0] >> env[1] >> env[2] >> k;
      const char* names[3] = {"GGRS_SCHED_SPLIT", "GGRS_SCHED_CHAINS", "GGRS_SCHED_K"};
      for (int v = 0; v < 3; v++) env[v] == "-" ? unsetenv(names[v]) : setenv(names[v], env[v].c_str(), 1);
      const SchedOverrides ov = sched_overrides_from_env();
      in.R = in.max_prediction + 1;
      in.sparse = sparse, in.desync = desync, in.peer_reports = reports, in.trace = trace;
      for (int a = 0; a < k && !failed; a++) {
        is >> in.left;
        printf("ADVANCE %d\n", in.left);
        in.cap_left = 0;
        while (in.left > 0) {
          SchedLaunch L, again;
          const char *msg = nullptr, *msg2 = nullptr;
          const int rc = sched_plan_next(in, ov, &L, &msg);
          if (sched_plan_next(in, ov, &again, &msg2) != rc || (rc == 0 && show(again, in, f0) != show(L, in, f0)))
            printf("UNSTABLE\n");
          if (rc) {
            printf("ERROR %d %s\n", rc, msg);
            failed = true;
            break;
          }
          printf("%s\n", show(L, in, f0).c_str());
          if (L.n < 1 || L.n > in.left) return 2;
          f0 += L.n, in.left -= L.n, in.cap_left = L.cap_left;
        }
      }
    } else {
      return 3;
    }
  }
  return 0;
}
