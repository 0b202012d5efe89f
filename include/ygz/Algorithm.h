#ifndef YGZ_ALGORITHM_H_
#define YGZ_ALGORITHM_H_
#include "ygz/Algorithm/FeatureDetector.h"
#include "ygz/Algorithm/Matcher.h"
#include "ygz/Algorithm/Tracker.h"
#include "ygz/Algorithm/SparseImageAlign.h"
#include "ygz/Algorithm/CVUtils.h"
#include "ygz/Algorithm/BA.h"
#include "ygz/Algorithm/Initializer.h"
#include "ygz/Algorithm/KeyFrameDatabase.h"
#include "ygz/Algorithm/KeyFrameCulling.h"
#include "ygz/Algorithm/Relocalizer.h"
#include "ygz/Algorithm/LoopClosing.h"
#include "ygz/Algorithm/StereoMatcher.h"
#include "ygz/Algorithm/PoseOptimizer.h"
#include "ygz/Algorithm/BundleAdjuster.h"
#include "ygz/Algorithm/StereoMapper.h"
#endif
