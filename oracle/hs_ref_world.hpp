// ORACLE — TEST INFRASTRUCTURE ONLY (see hs_ref_math.hpp header).
// Per-world state of the CPU restatement.  Mirrors `struct Sim` (src/sim.hpp:315-363) and the
// ECS columns it touches, flattened into fixed-capacity slot tables (SURVEY §7 design stance).
#pragma once
#include "hs_ref_math.hpp"
#include "hs_ref_rng.hpp"

namespace hsref {

// Capacities, the slot layout of movable ("D") bodies (boxes, then ramps, then agents) and the SimObject / OwnerTeam /
// ResponseType / AgentType / SimFlags values are the scalar core's (csrc/hs_core.h).
// The reference's worst case is 34 walls (geo_gen.cpp:429-462; its TmpArray holds 33 and the
// overflow is only asserted in debug builds, geo_gen.cpp:24,144-147); kMaxWalls holds 36.

struct DBody {
    int32_t objType;       // SimObject or OBJ_NONE when the slot is empty
    int32_t response;      // ResponseType
    int32_t owner;         // OwnerTeam
    V3 pos; Q rot;
    V3 lin, ang;           // Velocity
    V3 extForce, extTorque;
    // substep scratch
    V3 prevPos; Q prevRot;
};

struct WallS { float cx, cy, hx, hy; };       // z in [0, 2.5]; half extents in x/y
struct PlaneS { V3 n; float d; };             // n.p = d

struct GrabJoint {                            // PhysicsSystem::makeFixedJoint (sim.cpp:354-356)
    int32_t other;                            // D-slot of the grabbed body, -1 when none
    V3 r1, r2; Q attach1, attach2; float separation;
};

struct World {
    // --- Sim fields (sim.hpp:326-362)
    uint32_t curWorldEpisode;
    RandKey curEpisodeRNDCounter;
    RNG rng;
    int32_t numHiders, numSeekers, numActiveAgents;
    int32_t hiders[3], seekers[3];            // agent indices (0..A-1)
    int32_t numActiveBoxes, numActiveRamps;
    V3 boxSizes[kMaxBoxes];
    int32_t curEpisodeStep;
    float hiderTeamReward;
    // --- singletons (sim.hpp:105-121)
    bool seekersFirst;
    int32_t runningScores[2];
    // --- bodies
    DBody d[kNumDSlots];
    int32_t numWalls; WallS walls[kMaxWalls];
    int32_t numPlanes; PlaneS planes[kMaxPlanes];
    // --- agent interface columns that are not exported tensors
    int32_t agentType[kMaxAgents];
    int32_t agentActive[kMaxAgents];          // SimEntity != none
    GrabJoint grab[kMaxAgents];
};

}  // namespace hsref
