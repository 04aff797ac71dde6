// mas_bot_rule.h -- the scripted bots' rule (include/masurvival.h, mas_bot_act)
// as host/device functions of scalars: what one lane group of k_bot_act
// (mas_bot.hip) evaluates once the row's fields and the nearest targets are in
// registers.  fp32, every operation rounded on its own (-ffp-contract=off),
// the heading from the shared double sincos of mas_math.h.
#pragma once

#include "mas_math.h"

namespace mas {
namespace bot {

constexpr int kIdle = 0, kHunter = 1, kForager = 2;  // MAS_BOT_*
constexpr float kZoneMargin = 1.0f;
constexpr float kTurnBand = 0.15f;
constexpr float kTurnDamp = 0.25f;
constexpr float kMoveCone = 0.8f;
constexpr float kAttackCone = 0.9f;
constexpr float kStandoff = 1.25f;
constexpr float kArrived = 0.25f;
constexpr float kForagerFight2 = 16.0f;  // 4 m, squared

// a candidate target of the nearest search: squared distance, index (its
// order among equals), position.  idx < 0: none
struct Cand {
    float d2;
    int idx;
    float x, y;
};
MAS_HD Cand no_cand()
{
    Cand c;
    c.d2 = 0.0f;
    c.idx = -1;
    c.x = 0.0f;
    c.y = 0.0f;
    return c;
}
// the nearer of two candidates; among equal squared distances the lowest
// index: a total order, so the result does not depend on the reduction's shape
MAS_HD Cand nearer(Cand a, Cand b)
{
    if (b.idx < 0) return a;
    if (a.idx < 0) return b;
    const bool take_b = b.d2 < a.d2 || (b.d2 == a.d2 && b.idx < a.idx);
    return take_b ? b : a;
}

MAS_HD float sq_dist(float ax, float ay, float bx, float by)
{
    const float dx = ax - bx, dy = ay - by;
    return dx * dx + dy * dy;
}

// the row's own fields and the call's thresholds
struct Self {
    float health, x, y, theta, w;
    float zx, zy, zr;
    float hsm;       // heal_slot_mask (n_heals > 0)
};
struct Rule {
    int kind, n_heals;
    float use_below;  // agent_health - healing
    float reach;      // melee_range + agent_size / 2
};

// m^2 of the zone test: m = max(zone_r - 1, 0)
MAS_HD float zone_m2(float zr)
{
    const float m0 = zr - kZoneMargin;
    const float m = m0 > 0.0f ? m0 : 0.0f;
    return m * m;
}

// The six action values packed as three 2-B words (a[0] | a[1] << 8, ...), from
// the row's fields, the nearest admissible heal (FORAGER; heals outside the
// zone's margin already left out) and the nearest admissible enemy.
MAS_HD void decide(const Rule& r, const Self& s, Cand heal, Cand enemy, uint16_t out[3])
{
    int a0 = 1, a2 = 1, a3 = 0, a4 = 0;
    if (r.kind != kIdle && s.health > 0.0f) {
        a4 = (r.n_heals > 0 && s.hsm == 0.0f && s.health <= r.use_below) ? 1 : 0;
        int tk = 0;  // 1 zone, 2 heal, 3 enemy
        float tx = 0.0f, ty = 0.0f;
        if (sq_dist(s.x, s.y, s.zx, s.zy) > zone_m2(s.zr)) {
            tk = 1, tx = s.zx, ty = s.zy;
        } else if (r.kind == kForager && heal.idx >= 0) {
            tk = 2, tx = heal.x, ty = heal.y;
        } else if (enemy.idx >= 0 && !(r.kind == kForager && enemy.d2 > kForagerFight2)) {
            tk = 3, tx = enemy.x, ty = enemy.y;
        }
        if (tk == 0) {
            a2 = 2;
        } else {
            const float dx = tx - s.x, dy = ty - s.y;
            const float l = sqrtf(dx * dx + dy * dy);
            const Rot h = rot_of(s.theta);
            const float c = h.c * dx + h.s * dy;
            const float sn = h.c * dy - h.s * dx;
            const float u = sn - (kTurnDamp * s.w) * l;
            const float b = kTurnBand * l;
            a2 = u > b ? 2 : (-b > u ? 0 : (0.0f > c ? 2 : 1));
            const float stop = tk == 3 ? kStandoff : kArrived;
            a0 = (c > kMoveCone * l && l > stop) ? 2 : 1;
            a3 = (tk == 3 && !(l > r.reach) && c > kAttackCone * l) ? 1 : 0;
        }
    }
    out[0] = (uint16_t)(a0 | (1 << 8));
    out[1] = (uint16_t)(a2 | (a3 << 8));
    out[2] = (uint16_t)a4;
}

}  // namespace bot
}  // namespace mas
