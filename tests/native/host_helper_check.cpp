// LocalBA's helper thread (csrc/host_helper.h) on its own: 1000 short jobs posted and waited for in
// sequence, each run exactly once with its writes visible when wait() returns; a helper destroyed with
// and without a job ever posted.  Built with ThreadSanitizer (a missing release / acquire pairing on the
// job's plain writes is a reported race) and with AddressSanitizer.  No fork.
#include <cstdio>
#include <vector>

#include "host_helper.h"

using orbamd_host::HostHelper;

int main() {
    int fails = 0;
    {
        HostHelper idle;   // never posted to: no thread was started, nothing to join
        idle.wait();       // (and nothing to wait for)
    }
    {
        constexpr int JOBS = 1000;
        HostHelper h;
        std::vector<int> ran(JOBS, 0);   // plain memory: written by the helper, read here after wait()
        long sum = 0;                    // likewise, carried from job to job
        for (int k = 0; k < JOBS; k++) {
            int* cell = &ran[k];
            long* s = &sum;
            h.post([cell, s, k] {
                *cell += 1;
                *s += k;
            });
            h.wait();
            if (ran[k] != 1 || sum != (long)k * (k + 1) / 2) fails++;
        }
        for (int k = 0; k < JOBS; k++)
            if (ran[k] != 1) fails++;
        h.wait();   // a second wait after a finished job returns at once
    }   // destroyed with its thread idle: joined
    {
        HostHelper h;
        int x = 0;
        h.post([&x] { x = 7; });
        h.wait();
        if (x != 7) fails++;
    }
    printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
