// Host mirror of mapOptimization's GPS handling up to the factor: gpsHandler (mapOptimization.cpp:334-337) and the
// decisions of addGPSFactor (:1430-1507).  The factor itself and the covariance that gates it are the library's
// (include/lvi_pgo_gps.h); this is a pure decision on a few floats, so it is host work and depends on nothing but the
// standard library (the CPU tier compiles it alone).
//
// addGPSFactor, in the reference's order:
//   1. no message queued                                                             -> nothing      (:1432-1433)
//   2. no key poses                                                                   -> nothing      (:1436-1437)
//   3. pointDistance(cloudKeyPoses3D.front(), back()) < 5.0 (float arithmetic, the key poses BEFORE the new key is pushed)
//                                                                                     -> nothing      (:1440-1441)
//   4. poseCovariance(3,3) < poseCovThreshold && poseCovariance(4,4) < poseCovThreshold -> nothing      (:1445-1446)
//   5. drain: pop every message older than timeLaserInfoCur - 0.2, stop at the first newer than timeLaserInfoCur + 0.2 (:1451-1462)
//   6. a message inside the window is popped and (:1464-1502)
//        skipped when noise_x or noise_y exceeds gpsCovThreshold (floats of covariance[0], [7]; noise_z = float(covariance[14])),
//        without useGpsElevation: gps_z = transformTobeMapped[5], noise_z = 0.01,
//        skipped when |x| < 1e-6 && |y| < 1e-6,
//        skipped when closer than 5 m to lastGPSPoint — a function-static in the reference that starts at (0, 0, 0), so a fix
//          within 5 m of the origin is skipped; the quirk is kept, as a member,
//        otherwise ONE GPSFactor(key, (x, y, z), Variances(max(noise, 1.0f) x3)) is returned and the drain stops: the rest of
//        the queue stays for the next key.
#pragma once
#include <algorithm>
#include <cmath>
#include <deque>

namespace lvi_host {

struct GpsSettings {                            // utility.h:178-183; params_lidar.yaml sets none of them
    bool  useGpsElevation = false;
    float gpsCovThreshold = 2.0f;
    float poseCovThreshold = 25.0f;
};

struct GpsMessage {                             // what addGPSFactor reads of the nav_msgs Odometry
    double stamp = 0.0;
    double x = 0.0, y = 0.0, z = 0.0;           // pose.pose.position
    double cov_x = 0.0, cov_y = 0.0, cov_z = 0.0;   // pose.covariance[0], [7], [14]
};

struct GpsFactor {                              // GPSFactor(key, Point3(xyz), Variances(variance)); the key is the caller's
    float xyz[3];
    float variance[3];
};

class GpsGate {
public:
    explicit GpsGate(const GpsSettings& s = GpsSettings()) : S(s) {}
    GpsSettings S;
    std::deque<GpsMessage> gpsQueue;
    float lastGPSPoint[3] = {0.f, 0.f, 0.f};
    int accepted = 0;                           // factors handed out so far

    void gpsHandler(const GpsMessage& m) { gpsQueue.push_back(m); }                       // :334-337

    // addGPSFactor (:1430-1507) for the key about to be pushed.  keyFront / keyBack: x, y, z of cloudKeyPoses3D.front() /
    // .back() (nullptr: no key poses); covXX / covYY: poseCovariance(3,3) / (4,4); tobeMappedZ: transformTobeMapped[5].
    // true: *out is the one factor to add (and aLoopIsClosed is to be set).
    bool addGPSFactor(double timeLaserInfoCur, const float* keyFront, const float* keyBack, double covXX, double covYY, float tobeMappedZ, GpsFactor* out)
    {
        if (gpsQueue.empty()) return false;
        if (!keyFront || !keyBack) return false;
        if (pointDistance(keyFront, keyBack) < 5.0) return false;
        if (covXX < S.poseCovThreshold && covYY < S.poseCovThreshold) return false;
        while (!gpsQueue.empty()) {
            if (gpsQueue.front().stamp < timeLaserInfoCur - 0.2) {
                gpsQueue.pop_front();                                                     // message too old
            } else if (gpsQueue.front().stamp > timeLaserInfoCur + 0.2) {
                break;                                                                    // message too new
            } else {
                const GpsMessage thisGPS = gpsQueue.front();
                gpsQueue.pop_front();
                float noise_x = (float)thisGPS.cov_x, noise_y = (float)thisGPS.cov_y, noise_z = (float)thisGPS.cov_z;
                if (noise_x > S.gpsCovThreshold || noise_y > S.gpsCovThreshold) continue; // GPS too noisy
                float gps_x = (float)thisGPS.x, gps_y = (float)thisGPS.y, gps_z = (float)thisGPS.z;
                if (!S.useGpsElevation) { gps_z = tobeMappedZ; noise_z = 0.01f; }
                if (std::fabs(gps_x) < 1e-6 && std::fabs(gps_y) < 1e-6) continue;          // GPS not properly initialised (0, 0, 0)
                const float cur[3] = {gps_x, gps_y, gps_z};
                if (pointDistance(cur, lastGPSPoint) < 5.0) continue;                     // a GPS factor every few metres
                for (int k = 0; k < 3; k++) lastGPSPoint[k] = cur[k];
                out->xyz[0] = gps_x; out->xyz[1] = gps_y; out->xyz[2] = gps_z;
                out->variance[0] = std::max(noise_x, 1.0f); out->variance[1] = std::max(noise_y, 1.0f); out->variance[2] = std::max(noise_z, 1.0f);
                accepted++;
                return true;
            }
        }
        return false;
    }

    static float pointDistance(const float a[3], const float b[3])                        // utility.h: sqrt of the float sum of squares
    {
        const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
        return std::sqrt((dx * dx + dy * dy) + dz * dz);
    }
};

}  // namespace lvi_host
