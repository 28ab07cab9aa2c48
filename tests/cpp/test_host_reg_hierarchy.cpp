// test_host_reg_hierarchy.cpp — the regularisation hierarchy through the host adaptor (DynFuParams::north_star_reg_hierarchy,
// reg_level_slots, and L, beta, epsilon, which it finally reads; NorthStarSolver::setRegHierarchy; DynFusion::northStarNodeLevels).
// The switch's rules; on the half-sphere sequence of test_host_regrow.cpp with the switch on: the levels are dfa_node_levels'
// on the field's nodes every frame, old nodes keep theirs as the field grows, the frames solve; with the switch off a
// sequence's outputs keep their bits — also after hierarchical runs have left their plans in the adaptor's cache.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include <dynfu/dyn_fusion.hpp>
#include <kfusion/cuda/tsdf_volume.hpp>

#include "../../include/dynfu_amd.h"
#include "dynfu_fixtures.hpp"
#include "minitest.hpp"

using namespace kfusion;
using namespace dynfu_fixtures;
using namespace dynfu_fixtures::sphere_scene;

namespace {
const int DIM = 64;

DynFuParams params(bool hierarchy) {
    DynFuParams p = DynFuParams::defaultParams();
    p.kinfuParams.cols = W, p.kinfuParams.rows = H;
    p.kinfuParams.intr = Intr(F, F, W / 2 - 0.5f, H / 2 - 0.5f);
    p.kinfuParams.volume_dims = Vec3i::all(DIM);
    p.epsilon = 0.05f;
    p.north_star = true, p.north_star_fuse_canonical = true;
    p.fuse_unsupported_rigid = true, p.north_star_regrow_canonical = true, p.canonical_min_weight = 2;
    p.north_star_reg_hierarchy = hierarchy;
    return p;
}

struct Depths {
    cuda::Depth d[4];
    Depths() {
        for (int f = 0; f < 4; ++f) d[f].upload(sphere_depth(1.5f - 0.01f * f, f == 0), W);  // 1 cm closer per frame
    }
};

// what a frame leaves: the warped cloud, the node arrays, the canonical volume, the energies
struct Outputs {
    std::vector<float> warped, pos, w, dq;
    std::vector<uint32_t> volume;
    double cost0 = 0, cost1 = 0;
    long long valid = 0;
};
Outputs outputs(DynFusion& df) {
    Outputs o;
    dfa::DeviceArray<float> v3, n3;
    df.getCanonicalWarpedToLive()->deviceArrays(v3, n3);
    if (df.getCanonicalWarpedToLive()->size()) v3.download(o.warped);
    df.getWarpfield()->hostArrays(o.pos, o.w, o.dq);
    o.volume.resize((size_t)DIM * DIM * DIM);
    df.canonicalVolume()->data().download(o.volume.data(), o.volume.size() * sizeof(uint32_t));
    o.cost0 = df.northStarInitialCost(), o.cost1 = df.northStarFinalCost(), o.valid = df.northStarValidRows();
    return o;
}
using dynfu_fixtures::same;  // (the overload below would hide it)
bool same(const Outputs& a, const Outputs& b) {
    return same(a.warped, b.warped) && same(a.pos, b.pos) && same(a.w, b.w) && same(a.dq, b.dq) && same(a.volume, b.volume) &&
           std::memcmp(&a.cost0, &b.cost0, sizeof(double)) == 0 && std::memcmp(&a.cost1, &b.cost1, sizeof(double)) == 0 &&
           a.valid == b.valid;
}
std::vector<Outputs> run(bool hierarchy, const Depths& in) {
    DynFusion df(params(hierarchy));
    df.nodeStep = 16;
    std::vector<Outputs> out;
    for (int f = 0; f < 4; ++f) {
        df(in.d[f]);
        if (f > 0) out.push_back(outputs(df));
    }
    return out;
}

// dfa_node_levels over the first D of the field's nodes
std::vector<int> levels_by_the_library(DynFusion& df, size_t D, float epsilon, int beta, int levels) {
    const Warpfield::DeviceNodeView nodes = df.getWarpfield()->deviceNodes();
    dfa::DeviceArray<int> out(D);
    dfa::check(dfa_node_levels(nodes.pos, (int)D, epsilon, beta, levels, out.ptr(), nullptr), "dfa_node_levels");
    std::vector<int> h;
    out.download(h);
    return h;
}
}  // namespace

TEST(RegHierarchyTest, ConstructorRules) {
    const DynFuParams def = DynFuParams::defaultParams();
    ASSERT_TRUE(!def.north_star_reg_hierarchy && def.reg_level_slots == (std::vector<int>{4, 2, 2}));
    ASSERT_TRUE(def.L == 4 && def.beta == 4);
    DynFuParams p = params(true);
    ASSERT_TRUE(!construction_throws(p));
    DynFuParams a = p;  // needs north_star
    a.north_star = a.north_star_fuse_canonical = a.north_star_regrow_canonical = a.fuse_unsupported_rigid = false;
    ASSERT_TRUE(construction_throws(a));
    DynFuParams b = p;  // more slots than the field's k
    b.reg_level_slots = {4, 3, 2};
    ASSERT_TRUE(construction_throws(b));
    b.L = 1;  // ... unless the levels used stop before them: min(L + 1, slots) = 2 levels, 7 slots
    ASSERT_TRUE(!construction_throws(b));
    DynFuParams c = p;
    c.reg_level_slots = {0, 2, 2};
    ASSERT_TRUE(construction_throws(c));
    c.reg_level_slots = {4, -1, 2};
    ASSERT_TRUE(construction_throws(c));
    c.reg_level_slots = {1, 1, 1, 1, 1, 1, 1, 1, 1}, c.L = 8;
    ASSERT_TRUE(construction_throws(c));
    c.reg_level_slots = {};
    ASSERT_TRUE(construction_throws(c));
    DynFuParams d = p;
    d.beta = 1;
    ASSERT_TRUE(construction_throws(d));
    d.beta = 4, d.epsilon = 0.f;
    ASSERT_TRUE(construction_throws(d));
    // the same refusals from the solver's own call
    NorthStarSolver solver(Warpfield(), NorthStarParameters(), 4.652f, 0.01f, 200.f, 1e-4f);
    bool threw = false;
    try {
        solver.setRegHierarchy({4, 3, 2}, 0.05f, 4);
    } catch (const dfa::Error& e) {
        threw = e.code == DFA_ERR_INVALID;
    }
    ASSERT_TRUE(threw);
    solver.setRegHierarchy({4, 2, 2}, 0.05f, 4);
    solver.setRegHierarchy({}, 0.f, 0);  // back to the flat graph: nothing to refuse
}

TEST(RegHierarchyTest, TheLevelsAreTheLibrarysAndOldNodesKeepTheirs) {
    Depths in;
    DynFuParams p = params(true);
    DynFusion df(p);
    df.nodeStep = 16;
    std::vector<int> before;
    size_t grown = 0;
    for (int f = 0; f < 4; ++f) {
        ASSERT_TRUE(df(in.d[f]) == (f > 0));
        if (f == 0) {
            ASSERT_TRUE(df.northStarNodeLevels().empty());
            continue;
        }
        const std::vector<int> counts = df.northStarNodeLevels(), each = df.northStarNodeLevelOfEach();
        ASSERT_EQ(counts.size(), (size_t)3);  // min(L + 1, reg_level_slots.size())
        ASSERT_EQ((size_t)std::accumulate(counts.begin(), counts.end(), 0), each.size());
        ASSERT_TRUE(each.size() > 5 && each.size() <= df.getWarpfield()->nodesRef().size());
        // the nodes the frame solved over are the first of the field as it is now (update only appends)
        const std::vector<int> want = levels_by_the_library(df, each.size(), p.epsilon, p.beta, 3);
        ASSERT_TRUE(same(each, want));
        ASSERT_TRUE(counts[1] + counts[2] > 0 && counts[0] > 0);  // (a few dozen nodes: some represent a coarse cell, some do not)
        if (!before.empty()) {
            ASSERT_TRUE(each.size() >= before.size());
            ASSERT_TRUE(std::equal(before.begin(), before.end(), each.begin()));
            grown += each.size() - before.size();
        }
        before = each;
        std::printf("frame %d: %zu nodes, levels %d / %d / %d, cost %.4g -> %.4g, %lld valid rows\n", f, each.size(), counts[0],
                    counts[1], counts[2], df.northStarInitialCost(), df.northStarFinalCost(), df.northStarValidRows());
        ASSERT_TRUE(std::isfinite(df.northStarFinalCost()) && df.northStarFinalCost() <= df.northStarInitialCost());
        ASSERT_TRUE(df.northStarValidRows() > 100);
    }
    ASSERT_TRUE(grown > 0);  // the field grew while the hierarchy was on
}

TEST(RegHierarchyTest, SwitchedOffASequenceKeepsItsBits) {
    Depths in;
    const std::vector<Outputs> flat0 = run(false, in);
    const std::vector<Outputs> hier  = run(true, in);   // leaves hierarchical plans in the adaptor's cache
    const std::vector<Outputs> flat1 = run(false, in);  // ... which a flat run takes
    ASSERT_EQ(flat0.size(), (size_t)3);
    bool differs = false;
    for (size_t f = 0; f < flat0.size(); ++f) {
        ASSERT_TRUE(same(flat0[f], flat1[f]));
        differs = differs || !same(flat0[f].dq, hier[f].dq);
    }
    ASSERT_TRUE(differs);  // (the switch does something)
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
