// input_demo.cpp -- the input-side adapters of include/ebvo/adapters.hpp as Pipeline::prepare_Stereo_Images and
// Stereo_Matches::augment_Edge_Data / apply_SIFT_filtering would call them (src/Pipeline.cpp:78-79,
// src/Stereo_Matches.cpp:655-787): ebvo::undistort, ebvo::sift_descriptors, ebvo::sift_min_distances, with plain local
// types standing where cv::Mat / struct Edge stand in the reference tree.
// usage: input_demo <in.bin> <out.bin>
// in.bin:  int32 h, w, n_dist; f64 K[4], dist[n_dist]; u8 image[h * w]                      (undistortion)
//          int32 h, w, n_edges; u8 image[h * w]; edges (x, y, theta as f64, index + pad as 2 i32)   (descriptors)
//          int32 n_pairs; int32 row_ptr[n_edges + 1]; int32 cand[n_pairs]   (distances: candidate k is edge cand[k])
// out.bin: u8 undistorted[h * w]; f32 descriptors[n_edges * 256]; f64 distances[n_pairs]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ebvo/adapters.hpp"

struct Point2d
{
    double x, y;
};
struct Edge
{
    Point2d location{-1.0, -1.0};
    double orientation = -100;
    bool b_isEmpty = true;
    int frame_source = -1;
    int index = 0;
};

template <class T>
static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n)
    {
        std::fprintf(stderr, "short input\n");
        std::exit(2);
    }
    return v;
}

template <class T>
static void put(FILE *f, const std::vector<T> &v)
{
    if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size())
        std::exit(2);
}

int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *in = std::fopen(argv[1], "rb");
    if (!in)
        return 2;
    // cv::undistort(image, undistorted, K, dist)
    auto hd = take<int32_t>(in, 3);
    const int h = hd[0], w = hd[1], n_dist = hd[2];
    auto K = take<double>(in, 4);
    auto dist = take<double>(in, (size_t)n_dist);
    auto img = take<uint8_t>(in, (size_t)h * w);
    // SIFT: image, edges, candidate lists
    auto hs = take<int32_t>(in, 3);
    const int sh = hs[0], sw = hs[1], n_edges = hs[2];
    auto simg = take<uint8_t>(in, (size_t)sh * sw);
    std::vector<Edge> edges((size_t)n_edges);
    for (auto &e : edges)
    {
        auto xyz = take<double>(in, 3);
        auto ip = take<int32_t>(in, 2);
        e.location = {xyz[0], xyz[1]};
        e.orientation = xyz[2];
        e.index = ip[0];
    }
    const int n_pairs = take<int32_t>(in, 1)[0];
    auto row_ptr = take<int32_t>(in, (size_t)n_edges + 1);
    auto cand = take<int32_t>(in, (size_t)n_pairs);
    std::fclose(in);

    ebvo::Context ctx(h > sh ? h : sh, w > sw ? w : sw);
    if (ctx.status() != EBVO_OK)
        return 3;
    std::vector<uint8_t> und = ebvo::undistort(ctx, img.data(), h, w, (ptrdiff_t)w, K.data(), dist);
    if (und.size() != (size_t)h * w)
        return 4;
    std::vector<float> desc = ebvo::sift_descriptors(ctx, simg.data(), sh, sw, (ptrdiff_t)sw, edges);
    if (desc.size() != (size_t)n_edges * 256)
        return 5;
    std::vector<float> cand_desc((size_t)n_pairs * 256);
    for (int k = 0; k < n_pairs; ++k)
        for (int q = 0; q < 256; ++q)
            cand_desc[(size_t)k * 256 + q] = desc[(size_t)cand[k] * 256 + q];
    std::vector<double> d = ebvo::sift_min_distances(ctx, desc, cand_desc, row_ptr);
    if (d.size() != (size_t)n_pairs)
        return 6;
    // a refused call leaves its output empty (six distortion coefficients)
    if (!ebvo::undistort(ctx, img.data(), h, w, (ptrdiff_t)w, K.data(), std::vector<double>(6, 0.0)).empty())
        return 7;

    FILE *out = std::fopen(argv[2], "wb");
    if (!out)
        return 2;
    put(out, und);
    put(out, desc);
    put(out, d);
    std::fclose(out);
    return 0;
}
