// Anti-entropy (p2pg_set_anti_entropy): the host's side of the periodic pull repair.
// An exchange of request round r takes three rounds: in r every online peer with a connection
// sends one request to one drawn connection, in r + 1 the partner answers, in r + 2 the reply
// arrives and what it lists is first-received.  Request rounds are the rounds r with
// first <= r <= last and (r - first) % period == 0.  Here: the one definition of "is r a request /
// reply / arrival round", "does one lie at or ahead of r" (what keeps a run going and what keeps
// p2pg_run from batching), and the validation of the three arguments.
//
// Plain C++: included by engine.cpp and by host programs (tests/test_anti_entropy_host.py).
#pragma once
#include <cstdint>

namespace anti_entropy {

// What is wrong with (first, last, period) (0: nothing).  period = 0 removes the setting: first and
// last are then not looked at.
enum Bad { OK = 0, BAD_PERIOD = 1, BAD_FIRST = 2, BAD_LAST = 3 };
inline Bad check(int32_t first, int32_t last, int32_t period) {
  if (period < 0) return BAD_PERIOD;
  if (period == 0) return OK;
  if (first < 0) return BAD_FIRST;
  if (last < first) return BAD_LAST;
  return OK;
}

struct Setting {
  int32_t first = 0, last = 0, period = 0;  // period 0: none set

  bool on() const { return period > 0; }
  // the last request round (on() only); 64-bit throughout: last may be INT32_MAX
  int64_t last_request() const {
    return (int64_t)first + ((int64_t)last - first) / period * period;
  }
  // Do the peers send their requests in round r?
  bool request_round(int64_t r) const {
    return on() && first <= r && r <= last && (r - first) % period == 0;
  }
  // Do the partners answer in round r (the requests of r - 1)?
  bool reply_round(int64_t r) const { return request_round(r - 1); }
  // Do the replies arrive in round r (the requests of r - 2)?  The only rounds that launch anything.
  bool arrival_round(int64_t r) const { return request_round(r - 2); }
  // Does a request round lie at or ahead of round r?
  bool request_ahead(int64_t r) const { return on() && r <= last_request(); }
  // Does an arrival round lie at or ahead of round r?  (A request round at or ahead, or an
  // exchange in flight: the run goes on, and p2pg_run does not batch across it.)
  bool arrival_ahead(int64_t r) const { return on() && r <= last_request() + 2; }
};

}  // namespace anti_entropy
