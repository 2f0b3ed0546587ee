// C++ API tests: the reference's own gtest cases (test/ProbabilisticWeightsTest.cc:35-66,
// test/PointCloudRegistrationTest.cc:30-116) restated against the drop-in classes, plus checks of the outer
// driver.  No gtest here: a tiny assert harness; exit code = number of failed checks.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <limits>
#include <memory>
#include <vector>

#include "prob_point_cloud_registration/prob_point_cloud_registration.h"
#include "prob_point_cloud_registration/utilities.hpp"

using namespace prob_point_cloud_registration;

// rho(1) of a term's loss = its weight (ScaledLoss(NULL, w): rho(s) = w s) — through ceres::LossFunction::Evaluate only
static double lossScale(const ceres::LossFunction *loss)
{
    double rho[3];
    loss->Evaluate(1.0, rho);
    return rho[0];
}

static int g_failed = 0, g_checks = 0;
#define EXPECT_NEAR(a, b, tol)                                                                            \
    do {                                                                                                  \
        ++g_checks;                                                                                       \
        const double a_ = (a), b_ = (b);                                                                  \
        if (!(std::fabs(a_ - b_) <= (tol))) {                                                             \
            ++g_failed;                                                                                   \
            std::printf("FAIL %s:%d: %s = %.12g, expected %.12g +- %g\n", __FILE__, __LINE__, #a, a_, b_, \
                        (double)(tol));                                                                   \
        }                                                                                                 \
    } while (0)
#define EXPECT_TRUE(c)                                                   \
    do {                                                                 \
        ++g_checks;                                                      \
        if (!(c)) {                                                      \
            ++g_failed;                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
        }                                                                \
    } while (0)

static Eigen::SparseMatrix<double, Eigen::RowMajor> dataAssociation()
{
    Eigen::SparseMatrix<double, Eigen::RowMajor> m(2, 4);
    std::vector<Eigen::Triplet<double>> t = {{0, 0, 1}, {0, 2, 1}, {0, 3, 1}, {1, 0, 1}, {1, 1, 1}, {1, 2, 1}, {1, 3, 1}};
    m.setFromTriplets(t.begin(), t.end());
    m.makeCompressed();
    return m;
}

static void weightsTests()
{
    const std::vector<double> sq = {1, 1, 1, 1, 4, 9, 16};
    const double expected_t[2][4] = {{1.0 / 3, 0, 1.0 / 3, 1.0 / 3}, {0.7151351, 0.1412613, 0.0241258, 0.0047656}};
    const double expected_g[2][4] = {{1.0 / 3, 0, 1.0 / 3, 1.0 / 3},
                                     {0.805153702921689, 0.179654074677018, 0.0147469044726408, 0.000445317928652638}};
    {
        ProbabilisticWeights w(5, 1, 4);
        auto out = w.updateWeights(dataAssociation(), sq);
        for (int i = 0; i < 2; i++)
            for (int j = 0; j < 4; j++) EXPECT_NEAR(expected_t[i][j], out.coeff(i, j), 1e-6);
    }
    {
        ProbabilisticWeights w(std::numeric_limits<double>::infinity(), 1, 4);
        auto out = w.updateWeights(dataAssociation(), sq);
        for (int i = 0; i < 2; i++)
            for (int j = 0; j < 4; j++) EXPECT_NEAR(expected_g[i][j], out.coeff(i, j), 1e-6);
    }
}

static pcl::PointCloud<pcl::PointXYZ> generateCloud()
{
    pcl::PointCloud<pcl::PointXYZ> cloud;
    double x = 0;
    for (int i = 0; i < 30; ++i) {
        double y = 0;
        for (int j = 0; j < 50; ++j) {
            cloud.push_back(pcl::PointXYZ((float)x, (float)y, (float)(std::sin(x) + std::cos(y))));
            y += 0.5;
        }
        x += 0.5;
    }
    return cloud;
}

static Eigen::Affine3d testTransform()
{
    // translation (2.5, 0, 0) then prerotate Rz(0.34): y = Rz (p + (2.5,0,0))
    Eigen::Affine3d T = Eigen::Affine3d::Identity();
    const double a = 0.34;
    T.linear()(0, 0) = std::cos(a), T.linear()(0, 1) = -std::sin(a), T.linear()(1, 0) = std::sin(a), T.linear()(1, 1) = std::cos(a);
    T.translation() = Eigen::Vector3d(2.5 * std::cos(a), 2.5 * std::sin(a), 0);
    return T;
}

static void exactAssociationTest(double dof)
{
    auto source = generateCloud();
    pcl::PointCloud<pcl::PointXYZ> target;
    pcl::transformPointCloud(source, target, testTransform());
    Eigen::SparseMatrix<double, Eigen::RowMajor> assoc(source.size(), target.size());
    std::vector<Eigen::Triplet<double>> tl;
    for (std::size_t i = 0; i < source.size(); ++i) tl.push_back(Eigen::Triplet<double>((int)i, (int)i, 1));
    assoc.setFromTriplets(tl.begin(), tl.end());
    assoc.makeCompressed();
    ProbPointCloudRegistrationParams params;
    params.dof = dof;
    params.max_neighbours = 3;
    ProbPointCloudRegistrationIteration registration(source, target, assoc, params);
    ceres::Solver::Options options;
    options.linear_solver_type = ceres::SPARSE_NORMAL_CHOLESKY;
    options.use_nonmonotonic_steps = true;
    options.max_num_iterations = std::numeric_limits<int>::max();
    options.function_tolerance = 10e-5;
    options.num_threads = 8;
    ceres::Solver::Summary summary;
    registration.solve(options, &summary);
    auto estimated = registration.transformation();
    pcl::PointCloud<pcl::PointXYZ> aligned;
    pcl::transformPointCloud(source, aligned, estimated);
    double mean_error = 0;
    for (std::size_t i = 0; i < target.size(); ++i)
        mean_error += std::sqrt(std::pow(target.at(i).x - aligned[i].x, 2) + std::pow(target.at(i).y - aligned[i].y, 2) +
                                std::pow(target.at(i).z - aligned[i].z, 2));
    mean_error /= target.size();
    EXPECT_NEAR(mean_error, 0, 1e-6);
    EXPECT_TRUE(summary.final_cost <= summary.initial_cost);
    EXPECT_TRUE(summary.num_successful_steps >= 1);
}

static void alignTest()
{
    // a jittered copy of the test surface, moved by a small known motion; full align() with kd-tree-free NN
    auto target = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>(generateCloud());
    Eigen::Affine3d T = Eigen::Affine3d::Identity();
    const double a = 0.02;
    T.linear()(0, 0) = std::cos(a), T.linear()(0, 1) = -std::sin(a), T.linear()(1, 0) = std::sin(a), T.linear()(1, 1) = std::cos(a);
    T.translation() = Eigen::Vector3d(0.05, -0.03, 0.02);
    auto source = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>();
    // source = T^-1 target
    Eigen::Affine3d Ti = Eigen::Affine3d::Identity();
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Ti.linear()(r, c) = T.linear()(c, r);
    for (int r = 0; r < 3; r++) Ti.translation()(r) = -(Ti.linear()(r, 0) * T.translation()(0) + Ti.linear()(r, 1) * T.translation()(1) + Ti.linear()(r, 2) * T.translation()(2));
    pcl::transformPointCloud(*target, *source, Ti);
    ProbPointCloudRegistrationParams params;
    params.radius = 0.4;
    params.max_neighbours = 5;
    params.n_iter = 30;
    params.summary = true;
    auto gt = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>(*target);
    const std::size_t n_before = target->size();
    ProbPointCloudRegistration reg(source, target, params, gt);
    reg.align();
    EXPECT_TRUE(target->size() == n_before);  // no target filter: caller's cloud untouched
    const auto hist = reg.transformation_history();
    EXPECT_TRUE(hist.size() >= 6 && hist.size() <= 30);  // earliest stop of hasConverged is after 6 iterations
    const auto est = reg.transformation();
    EXPECT_NEAR(est.translation().x(), 0.05, 2e-3);
    EXPECT_NEAR(est.translation().y(), -0.03, 2e-3);
    EXPECT_NEAR(est.translation().z(), 0.02, 2e-3);
    EXPECT_NEAR(est.rotation()(1, 0), std::sin(a), 1e-3);
    const std::string rep = reg.report();
    EXPECT_TRUE(rep.find("iter, n_success_steps, initial_cost, final_cost, tx, ty, tz, roll, pitch, yaw, mse_prev_iter, mse_gtruth") == 0);
    std::size_t lines = 0;
    for (char ch : rep) lines += ch == '\n';
    EXPECT_TRUE(lines == hist.size() + 1);
    // n_iter caps the loop; cost_drop_thresh = 0 runs exactly n_iter
    params.n_iter = 4;
    params.cost_drop_thresh = 0;
    params.summary = false;
    ProbPointCloudRegistration reg2(source, target, params);
    reg2.align();
    EXPECT_TRUE(reg2.transformation_history().size() == 4);
    // filters: the caller's target IS filtered in place, the source copy is not the caller's
    auto target2 = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>(*target);
    params.target_filter_size = 1.0;
    params.source_filter_size = 1.0;
    const std::size_t src_n = source->size();
    ProbPointCloudRegistration reg3(source, target2, params);
    EXPECT_TRUE(target2->size() < n_before && target2->size() > 0);
    EXPECT_TRUE(source->size() == src_n);
    reg3.align();
    EXPECT_TRUE(reg3.transformation_history().size() == 4);
}

static void errorTermTest()
{
    ErrorTerm e(pcl::PointXYZ(1, 0, 0), pcl::PointXYZ(0.5f, 1, 0));
    const double q[4] = {3.7 * std::cos(M_PI / 4), 0, 0, 3.7 * std::sin(M_PI / 4)};  // un-normalised Rz(90 deg)
    const double t[3] = {0.5, 0, 0};
    double r[3];
    e(q, t, r);  // R x = (0,1,0); + t = (0.5,1,0); y - that = 0
    EXPECT_NEAR(r[0], 0, 1e-12);
    EXPECT_NEAR(r[1], 0, 1e-12);
    EXPECT_NEAR(r[2], 0, 1e-12);
    e.updateWeight(0.25);
    EXPECT_NEAR(lossScale(static_cast<const ErrorTerm &>(e).weight()), 0.25, 0);
}

// Ownership of the loss wrapper as in the reference (error_term.hpp:17-19,45; ..._iteration.hpp:42-44): the reference's term
// never deletes the wrapper — the ceres::Problem it is added to does (TAKE_OWNERSHIP by default).  Here: a wrapper nobody
// took is freed with the last copy of the term; one that weight() handed out belongs to whoever took it (the stand-in
// "problem" below deletes it, as a real ceres::Problem would) and is not freed a second time.  A loss that counts its
// own destruction is put behind the wrapper to see who deleted what.
namespace {
int g_counting_loss_deleted = 0;
class CountingLoss : public ceres::LossFunction {
public:
    ~CountingLoss() override { ++g_counting_loss_deleted; }
    void Evaluate(double s, double out[3]) const override { out[0] = s, out[1] = 1.0, out[2] = 0.0; }
};
}  // namespace
static void errorTermOwnershipTest()
{
    g_counting_loss_deleted = 0;
    {   // never handed out: the term cleans up after itself
        ErrorTerm e(pcl::PointXYZ(1, 0, 0), pcl::PointXYZ(0, 1, 0));
        const_cast<ceres::LossFunctionWrapper *>(static_cast<const ErrorTerm &>(e).weight())->Reset(new CountingLoss, ceres::TAKE_OWNERSHIP);
        ErrorTerm copy(e);  // copies share the one wrapper (the reference's copies share its raw pointer)
        EXPECT_TRUE(static_cast<const ErrorTerm &>(copy).weight() == static_cast<const ErrorTerm &>(e).weight());
    }
    EXPECT_TRUE(g_counting_loss_deleted == 1);
    g_counting_loss_deleted = 0;
    ceres::LossFunctionWrapper *taken = nullptr;
    {   // handed out (through a copy): the taker owns it, neither the term nor its copy deletes it
        ErrorTerm e(pcl::PointXYZ(1, 0, 0), pcl::PointXYZ(0, 1, 0));
        ErrorTerm copy(e);
        taken = copy.weight();  // what problem.AddResidualBlock(cost, term.weight(), ...) receives
        taken->Reset(new CountingLoss, ceres::TAKE_OWNERSHIP);
        e.updateWeight(0.5);    // (replaces the counting loss: one deletion, by Reset)
        EXPECT_TRUE(g_counting_loss_deleted == 1);
        taken->Reset(new CountingLoss, ceres::TAKE_OWNERSHIP);
    }
    EXPECT_TRUE(g_counting_loss_deleted == 1);  // both terms are gone, the wrapper is not
    delete taken;                               // the "problem" goes away
    EXPECT_TRUE(g_counting_loss_deleted == 2);
}

// weight_updater_callback.hpp:15-64 driven the way ..._iteration.hpp:37-49 drives it: one ErrorTerm per nonzero of the
// association, the callback called with an empty summary; every term's weight must be what ProbabilisticWeights gives
// for the squared residuals of the terms themselves (evaluated here through the functor).  Both routes of the class.
static void weightUpdaterCallbackTest(double dof)
{
    auto source = generateCloud();
    pcl::PointCloud<pcl::PointXYZ> target;
    pcl::transformPointCloud(source, target, testTransform());
    // three target candidates per source point (its own image and two neighbours), empty rows in between
    const int rows = 200;
    Eigen::SparseMatrix<double, Eigen::RowMajor> assoc(rows, (long)target.size());
    std::vector<Eigen::Triplet<double>> tl;
    for (int i = 0; i < rows; ++i) {
        if (i % 7 == 3) continue;
        for (int d = 0; d < 1 + i % 3; ++d) tl.push_back(Eigen::Triplet<double>(i, (i * 5 + d * 11) % (int)target.size(), 1));
    }
    assoc.setFromTriplets(tl.begin(), tl.end());
    assoc.makeCompressed();
    ProbPointCloudRegistrationParams params;
    params.dof = dof;
    std::vector<std::unique_ptr<ErrorTerm>> owned;
    std::vector<ErrorTerm *> terms;
    for (long i = 0; i < assoc.outerSize(); ++i)
        for (Eigen::SparseMatrix<double, Eigen::RowMajor>::InnerIterator it(assoc, i); it; ++it) {
            owned.emplace_back(new ErrorTerm(source[(std::size_t)it.row()], target[(std::size_t)it.col()]));
            terms.push_back(owned.back().get());
        }
    double rotation[4] = {1.9 * std::cos(0.15), 0, 0, 1.9 * std::sin(0.15)};  // un-normalised Rz(0.3)
    double translation[3] = {2.3, 0.4, -0.1};
    ProbabilisticWeights weight_updater(dof, 3, params.max_neighbours);
    std::vector<double> sq;
    for (ErrorTerm *e : terms) {
        double r[3];
        (*e)(rotation, translation, r);
        sq.push_back(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    }
    const auto expected = weight_updater.updateWeights(assoc, sq);
    {
        WeightUpdaterCallback callback(&assoc, &params, &terms, &weight_updater, rotation, translation);
        EXPECT_TRUE(callback(ceres::IterationSummary()) == ceres::SOLVER_CONTINUE);
        EXPECT_TRUE(callback.onDevice());  // rows share their source point: K2 on the device
        for (std::size_t k = 0; k < terms.size(); ++k) EXPECT_NEAR(lossScale(static_cast<const ErrorTerm *>(terms[k])->weight()), expected.valuePtr()[k], 1e-12);
        // the pose is read through the pointers at every call (the reference's callback sees Ceres' live state)
        translation[0] += 0.25;
        callback(ceres::IterationSummary());
        sq.clear();
        for (ErrorTerm *e : terms) {
            double r[3];
            (*e)(rotation, translation, r);
            sq.push_back(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        }
        const auto moved = weight_updater.updateWeights(assoc, sq);
        for (std::size_t k = 0; k < terms.size(); ++k) EXPECT_NEAR(lossScale(static_cast<const ErrorTerm *>(terms[k])->weight()), moved.valuePtr()[k], 1e-12);
    }
    {
        // a row whose terms hold different source points cannot be one row of a device association: host residuals
        ErrorTerm odd(source[199], target[0]);
        ErrorTerm *keep = terms[1];
        terms[1] = &odd;
        WeightUpdaterCallback callback(&assoc, &params, &terms, &weight_updater, rotation, translation);
        callback(ceres::IterationSummary());
        EXPECT_TRUE(!callback.onDevice());
        sq.clear();
        for (ErrorTerm *e : terms) {
            double r[3];
            (*e)(rotation, translation, r);
            sq.push_back(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        }
        const auto mixed = weight_updater.updateWeights(assoc, sq);
        for (std::size_t k = 0; k < terms.size(); ++k) EXPECT_NEAR(lossScale(static_cast<const ErrorTerm *>(terms[k])->weight()), mixed.valuePtr()[k], 1e-15);
        terms[1] = keep;
    }
    {
        WeightUpdaterCallback callback(&assoc, &params, &terms, &weight_updater, rotation, translation);
        callback(ceres::IterationSummary());
        EXPECT_TRUE(callback.onDevice());
        // The caller rebuilds its association and terms between two calls (fewer rows, fewer terms), as the reference's
        // callback — which re-reads both at every call — allows: the device snapshot must be dropped, not written past.
        Eigen::SparseMatrix<double, Eigen::RowMajor> smaller(rows / 2, (long)target.size());
        std::vector<Eigen::Triplet<double>> tl2;
        for (int i = 0; i < rows / 2; ++i)
            for (int d = 0; d < 1 + (i + 1) % 2; ++d) tl2.push_back(Eigen::Triplet<double>(i, (i * 3 + d * 17) % (int)target.size(), 1));
        smaller.setFromTriplets(tl2.begin(), tl2.end());
        smaller.makeCompressed();
        std::vector<std::unique_ptr<ErrorTerm>> owned2;
        const std::vector<ErrorTerm *> before = terms;
        terms.clear();
        for (long i = 0; i < smaller.outerSize(); ++i)
            for (Eigen::SparseMatrix<double, Eigen::RowMajor>::InnerIterator it(smaller, i); it; ++it) {
                owned2.emplace_back(new ErrorTerm(source[(std::size_t)it.row()], target[(std::size_t)it.col()]));
                terms.push_back(owned2.back().get());
            }
        EXPECT_TRUE(terms.size() < before.size());
        assoc = smaller;
        callback(ceres::IterationSummary());
        EXPECT_TRUE(callback.onDevice());
        sq.clear();
        for (ErrorTerm *e : terms) {
            double r[3];
            (*e)(rotation, translation, r);
            sq.push_back(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        }
        const auto rebuilt = weight_updater.updateWeights(assoc, sq);
        for (std::size_t k = 0; k < terms.size(); ++k) EXPECT_NEAR(lossScale(static_cast<const ErrorTerm *>(terms[k])->weight()), rebuilt.valuePtr()[k], 1e-12);
    }
}

// utilities.hpp:28-234: closest-point metrics against a brute-force nearest neighbour computed right here
static void closestPointMetricsTest()
{
    auto a = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>();
    auto b = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>();
    unsigned s = 12345u;
    auto rnd = [&]() {
        s = s * 1664525u + 1013904223u;
        return (float)((s >> 8) & 0xFFFF) / 65536.0f;
    };
    for (int i = 0; i < 901; i++) b->push_back(pcl::PointXYZ(10 * rnd(), 7 * rnd(), 3 * rnd()));
    for (int i = 0; i < 401; i++) a->push_back(pcl::PointXYZ(12 * rnd() - 1, 9 * rnd() - 1, 5 * rnd() - 1));
    a->push_back(pcl::PointXYZ(500.f, -300.f, 80.f));  // far outlier
    std::vector<double> d;
    for (const auto &p : a->points) {
        float best = INFINITY;
        for (const auto &q : b->points) {
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            float v = dx * dx;
            v = v + dy * dy;
            v = v + dz * dz;
            best = std::fmin(best, v);
        }
        d.push_back(best);
    }
    double sum = 0;
    for (double v : d) sum += v;
    EXPECT_NEAR(sumSquaredError(a, b), sum, 1e-9 * sum);
    EXPECT_NEAR(averageClosestDistance(a, b), sum / d.size(), 1e-9 * sum);
    std::vector<double> sd = d;
    std::sort(sd.begin(), sd.end());
    const std::size_t n = sd.size();  // 402: even -> (sd[n/2] + sd[n/2+1]) / 2, the reference's convention
    const double med = (sd[n / 2] + sd[n / 2 + 1]) / 2.0;
    EXPECT_NEAR(medianClosestDistance(a, b), med, 1e-6 * med);
    double rs = 0;
    int nf = 0;
    for (double v : sd)
        if (v <= med * 3 && v >= med / 3) {
            rs += v;
            nf++;
        }
    EXPECT_TRUE(nf >= 10);
    EXPECT_NEAR(robustSumSquaredError(a, b), rs, 1e-6 * rs);
    EXPECT_NEAR(robustSumSquaredError(a, b, 3.0), rs, 1e-6 * rs);
    EXPECT_NEAR(robustAveragedSumSquaredError(a, b), rs / nf, 1e-6 * rs / nf);
    EXPECT_TRUE(robustSumSquaredError(a, b, 1.0000001) == std::numeric_limits<double>::max() ||
                robustSumSquaredError(a, b, 1.0000001) < rs);
    EXPECT_TRUE(robustMedianClosestDistance(a, b) > 0);
}

// utilities.hpp:236-263: host-only helpers (median of the stored d2 with the reference's index convention, Euler
// angles -> quaternion as Rz(yaw) * Ry(pitch) * Rx(roll))
static void hostUtilitiesTest()
{
    std::vector<Eigen::Triplet<double>> odd = {{0, 0, 5.0}, {0, 1, 1.0}, {1, 0, 4.0}, {1, 1, 2.0}, {2, 2, 3.0}};
    EXPECT_NEAR(medianDistance(odd), 4.0, 0);  // sorted 1 2 3 4 5, element (5 + 1) / 2 = 3 -> 4
    std::vector<Eigen::Triplet<double>> even = {{0, 0, 6.0}, {0, 1, 1.0}, {1, 0, 4.0}, {1, 1, 2.0}, {2, 2, 3.0}, {2, 0, 5.0}};
    EXPECT_NEAR(medianDistance(even), 4.5, 0);  // sorted 1..6, (element 3 + element 4) / 2 = (4 + 5) / 2
    const double roll = 0.3, pitch = -0.7, yaw = 1.1;
    const Eigen::Quaterniond q = euler2Quaternion(roll, pitch, yaw);
    EXPECT_NEAR(q.w() * q.w() + q.x() * q.x() + q.y() * q.y() + q.z() * q.z(), 1.0, 1e-15);
    const Eigen::Matrix3d R = q.toRotationMatrix();
    const double cr = std::cos(roll), sr = std::sin(roll), cp = std::cos(pitch), sp = std::sin(pitch), cy = std::cos(yaw),
                 sy = std::sin(yaw);
    const double want[3][3] = {{cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr},
                               {sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr},
                               {-sp, cp * sr, cp * cr}};
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) EXPECT_NEAR(R(a, b), want[a][b], 1e-15);
    EXPECT_NEAR(euler2Quaternion(0, 0, 0).w(), 1.0, 0);
    const Eigen::Quaterniond qz = euler2Quaternion(0, 0, M_PI / 2);
    EXPECT_NEAR(qz.z(), std::sqrt(0.5), 1e-15);
}

// The class's align() is ONE call into the device-paced loop (ppcr_align_report): its history must be, bit for bit, the
// history ppcr_align returns for the same clouds and parameters — for one inner step per association and for the
// reference's schedule (inner loop to function_tolerance), with and without the reports that -g / --dump ask for.
static void alignIsTheDevicePacedLoop()
{
    auto target = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>(generateCloud());
    auto source = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>();
    Eigen::Affine3d Ti = Eigen::Affine3d::Identity();
    const double a = -0.015;
    Ti.linear()(0, 0) = std::cos(a), Ti.linear()(0, 1) = -std::sin(a), Ti.linear()(1, 0) = std::sin(a), Ti.linear()(1, 1) = std::cos(a);
    Ti.translation() = Eigen::Vector3d(-0.04, 0.02, -0.03);
    pcl::transformPointCloud(*target, *source, Ti);
    for (int inner : {1, 100})
        for (int dof : {5, 3, 10})
            for (bool reports : {false, true}) {
                ProbPointCloudRegistrationParams params;
                params.radius = 0.4;
                params.max_neighbours = 5;
                params.n_iter = 7;
                params.cost_drop_thresh = 0;
                params.dof = dof;
                params.inner_max_steps = inner;
                params.summary = reports;
                std::vector<Eigen::Affine3d> hist;
                if (reports) {
                    auto gt = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>(*target);
                    ProbPointCloudRegistration reg(source, target, params, gt);
                    reg.align();
                    hist = reg.transformation_history();
                    std::size_t lines = 0;
                    for (char ch : reg.report()) lines += ch == '\n';
                    EXPECT_TRUE(lines == hist.size() + 1);
                } else {
                    ProbPointCloudRegistration reg(source, target, params);
                    reg.align();
                    hist = reg.transformation_history();
                    EXPECT_TRUE(reg.hasConverged());  // asking again after align() gives the same verdict
                }
                EXPECT_TRUE(hist.size() == 7);
                ppcr_ctx *ctx = nullptr;
                EXPECT_TRUE(ppcr_create(0, &ctx) == PPCR_OK);
                ppcr_set_params(ctx, params.radius, params.max_neighbours, params.dof, 3);
                ppcr_set_target(ctx, &(*target)[0].x, (int64_t)target->size(), sizeof(pcl::PointXYZ));
                ppcr_set_source(ctx, &(*source)[0].x, (int64_t)source->size(), sizeof(pcl::PointXYZ));
                std::vector<double> H(12 * 7);
                int done = 0;
                EXPECT_TRUE(ppcr_align(ctx, 7, 0.0, params.n_cost_drop_it, params.initial_rotation, params.initial_translation,
                                       inner, 10e-6, H.data(), nullptr, nullptr, &done) == PPCR_OK);
                EXPECT_TRUE(done == 7);
                // the class composes the increments itself (delta * previous): same products, same order -> same bits
                for (std::size_t k = 0; k < hist.size() && k < 7; k++)
                    for (int r = 0; r < 3; r++) {
                        for (int c = 0; c < 3; c++) EXPECT_NEAR(hist[k].rotation()(r, c), H[12 * k + 4 * r + c], 0);
                        EXPECT_NEAR(hist[k].translation()(r), H[12 * k + 4 * r + 3], 0);
                    }
                ppcr_destroy(ctx);
            }
}

// --bench: the throughput a user of the C++ classes sees (bench.py's `cpp_api` block).  Clouds come as raw float32 xyz
// triples; every measurement constructs a ProbPointCloudRegistration (upload, filters: not timed) and times align().
// Steady-state rate = S / (align time with warm + S iterations - align time with warm iterations), S = 3 x steps: both runs
// pay the same cold start (grid build, source sort, first associations), the difference is `steps` steady iterations.
static bool readCloud(const char *path, pcl::PointCloud<pcl::PointXYZ> &cloud)
{
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<float> xyz((std::size_t)bytes / 4);
    const std::size_t got = std::fread(xyz.data(), 4, xyz.size(), f);
    std::fclose(f);
    if (got != xyz.size() || xyz.size() % 3) return false;
    cloud.points.resize(xyz.size() / 3);
    for (std::size_t i = 0; i < cloud.points.size(); i++) cloud.points[i] = pcl::PointXYZ(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    return true;
}

static int benchMain(int argc, char **argv)
{
    if (argc < 10) {
        std::fprintf(stderr, "usage: %s --bench src.f32 tgt.f32 radius max_neighbours dof warm steps inner_max_steps [repeats]\n", argv[0]);
        return 2;
    }
    auto source = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>();
    auto target = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>();
    if (!readCloud(argv[2], *source) || !readCloud(argv[3], *target)) {
        std::fprintf(stderr, "cannot read the clouds\n");
        return 2;
    }
    ProbPointCloudRegistrationParams params;
    params.radius = std::atof(argv[4]);
    params.max_neighbours = std::atoi(argv[5]);
    params.dof = std::strcmp(argv[6], "inf") == 0 ? std::numeric_limits<double>::infinity() : std::atof(argv[6]);
    const int warm = std::atoi(argv[7]), steps = std::atoi(argv[8]);
    params.inner_max_steps = std::atoi(argv[9]);
    const int repeats = argc > 10 ? std::atoi(argv[10]) : 5;
    params.cost_drop_thresh = -1;  // exactly n_iter iterations, also once the registration has converged (-c 0 stops there)
    // every object is constructed (clouds uploaded) before anything is timed, and the align() calls then run back to
    // back: the device does not idle (and clock down) through uploads between two measurements
    std::vector<double> construct_s;
    auto make = [&](int n_iter) {
        params.n_iter = n_iter;
        const auto t0 = std::chrono::steady_clock::now();
        auto reg = std::make_unique<ProbPointCloudRegistration>(source, target, params);
        construct_s.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        return reg;
    };
    auto timed = [&](ProbPointCloudRegistration &reg, std::size_t *n_done) {
        const auto t0 = std::chrono::steady_clock::now();
        reg.align();
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (n_done) *n_done = reg.transformation_history().size();
        return dt;
    };
    std::vector<std::unique_ptr<ProbPointCloudRegistration>> warmups, shorts, longs;
    // the long run carries 3 x steps steady iterations: the difference of two cold starts (~1 ms each, +-0.1 ms) is
    // then small against what is measured
    const int steady_steps = 3 * steps;
    for (int k = 0; k < 3; k++) warmups.push_back(make(warm + steady_steps));
    for (int r = 0; r < repeats; r++) {
        shorts.push_back(make(warm));
        longs.push_back(make(warm + steady_steps));
    }
    std::size_t done = 0;
    for (auto &w : warmups) (void)timed(*w, &done);  // code objects, allocations, clocks
    std::vector<double> steady, whole, short_s;
    for (int r = 0; r < repeats; r++) {
        const double ta = timed(*shorts[(std::size_t)r], nullptr);
        short_s.push_back(ta);
        const double tb = timed(*longs[(std::size_t)r], &done);
        if (done != (std::size_t)(warm + steady_steps)) {
            std::fprintf(stderr, "early stop: %zu iterations\n", done);
            return 1;
        }
        steady.push_back(steady_steps / (tb - ta));
        whole.push_back((warm + steady_steps) / tb);
    }
    std::sort(steady.begin(), steady.end());
    std::sort(whole.begin(), whole.end());
    std::sort(short_s.begin(), short_s.end());
    std::sort(construct_s.begin(), construct_s.end());
    // what a fresh object's align() costs beyond its iterations at the steady rate (grid build, source sort, first
    // associations without cut-offs, allocations), and what constructing the object costs (uploads, early grid build)
    const double steady_med = steady[steady.size() / 2];
    const double fixed_ms = (short_s[short_s.size() / 2] - warm / steady_med) * 1e3;
    std::printf("{\"steady_it_per_s\": %.3f, \"steady_min\": %.3f, \"steady_max\": %.3f, \"whole_align_it_per_s\": %.3f, "
                "\"align_fixed_overhead_ms\": %.4f, \"construct_ms\": %.4f, "
                "\"warm\": %d, \"steps\": %d, \"inner_max_steps\": %d, \"repeats\": %d, \"points\": [%zu, %zu]}\n",
                steady_med, steady.front(), steady.back(), whole[whole.size() / 2], fixed_ms, construct_s[construct_s.size() / 2] * 1e3,
                warm, steady_steps, params.inner_max_steps, repeats, source->size(), target->size());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::string(argv[1]) == "--bench") return benchMain(argc, argv);
    hostUtilitiesTest();
    weightsTests();
    closestPointMetricsTest();
    exactAssociationTest(std::numeric_limits<double>::infinity());
    exactAssociationTest(5);
    errorTermTest();
    errorTermOwnershipTest();
    weightUpdaterCallbackTest(5);
    weightUpdaterCallbackTest(std::numeric_limits<double>::infinity());
    alignTest();
    alignIsTheDevicePacedLoop();
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed;
}
