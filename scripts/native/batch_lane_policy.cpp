// batch_lane_policy.cpp -- the lane rule of csrc/batch_lanes.h driven from a script of creations and destructions, as host code
// (tests/test_batch_lane_policy.py builds and runs it; no GPU).  Input, one command per line:
//     q <hw_queues>   start over with lane_count(hw_queues) empty lanes; prints "lanes <L>"
//     c <id>          batch <id> is created; prints "lane <l> loads <load[0]> ... <load[L-1]>"
//     d <id>          batch <id> is destroyed; prints the same line with the lane it leaves
// The bookkeeping around pick_lane (a load per lane, the lane of every batch) is the pool's in api_batch.hip.
#include <cstdio>
#include <map>

#include "batch_lanes.h"

int main() {
    int load[vp8::MAX_LANES] = {}, lanes = 0;
    std::map<int, int> lane_of;
    char op;
    int arg;
    auto line = [&](int l) {
        printf("lane %d loads", l);
        for (int i = 0; i < lanes; ++i) printf(" %d", load[i]);
        printf("\n");
    };
    while (scanf(" %c %d", &op, &arg) == 2) {
        if (op == 'q') {
            lanes = vp8::lane_count(arg);
            for (int &l : load) l = 0;
            lane_of.clear();
            printf("lanes %d\n", lanes);
        } else if (op == 'c') {
            const int l = vp8::pick_lane(load, lanes);
            if (l < 0 || lane_of.count(arg)) return 2;
            ++load[l];
            lane_of[arg] = l;
            line(l);
        } else if (op == 'd') {
            const auto it = lane_of.find(arg);
            if (it == lane_of.end()) return 2;
            const int l = it->second;
            --load[l];
            lane_of.erase(it);
            line(l);
        } else {
            return 2;
        }
    }
    return 0;
}
