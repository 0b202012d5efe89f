// Two properties of Matcher::FindDirectProjection's memo that need no device (neither path reaches Runtime::ctx()).  Written against include/ygz only.
// 1. The MapPoint overload, for a map point with no observation in `ref`, returns false and leaves mp->_obs as it was (no null entry for
//    ba::LocalBAG2O to dereference later).  Prints "miss <returned> <entries for ref> <entries>".
// 2. A Frame that outlives the Runtime -- a global, constructed before the Runtime's static and so destroyed after it -- is destroyed without
//    touching the Runtime or its memo.  The program exits with status 0.
// Built and run by tests/test_fdp_memo_host.py.
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
#include "ygz/hip/Runtime.h"
#include <cstdio>
using namespace ygz;

Frame g_outlives_runtime;

int main()
{
    hip::ResetFdpMemoStats();                     // the Runtime (and its memo) come to life here, after g_outlives_runtime
    Frame ref, other, curr;
    ref._keyframe_id = 3; other._keyframe_id = 4;
    Feature seen_elsewhere(Vector2d(100, 120), 0);
    seen_elsewhere._frame = &other;
    MapPoint mp;
    mp._obs[other._keyframe_id] = &seen_elsewhere;
    Matcher matcher;
    Vector2d px(110, 125);
    int level = -1;
    const bool found = matcher.FindDirectProjection(&ref, &curr, &mp, px, level);
    printf("miss %d %zu %zu\n", found ? 1 : 0, mp._obs.count(ref._keyframe_id), mp._obs.size());
    return 0;
}
