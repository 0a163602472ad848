// RtNearest.cs — K-nearest point queries (include/rt.h "K-nearest queries"): Physics.OverlapSphere over the EXISTING imports of
// RtNative.cs — rt_set_option("closest_k", K) and ("closest_all", 0 / 1), rt_closest_points, and both options back to 1 and 0 in a
// finally.  No new DllImport and no new record: the results are RtClosest (RtClosest.cs), K per point, point-major, nearest first, the
// unused ones miss records; _reserved[0] of every record of a point is the count.  The options go back to their defaults, not to what
// they were: a caller who has set them on the context themselves finds them cleared after either helper.
using System;

namespace RtMi355x
{
    public static class RtNearest
    {
        public const int MaxK = 8;      // RT_HITS_MAX

        // points: the point in origin, the search radius in tMax.  countAll: the count is every surface within the radius, not min(found, k).
        public static RtClosest[] NearestK(IntPtr ctx, RtRay[] points, int k = 4, bool countAll = false)
        {
            if (points == null) throw new ArgumentNullException(nameof(points));
            if (k < 1 || k > MaxK) throw new ArgumentOutOfRangeException(nameof(k), "k: 1..8");
            var result = new RtClosest[points.Length * k];
            try
            {
                RtNative.Check(ctx, RtNative.rt_set_option(ctx, "closest_k", k), "rt_set_option(closest_k)");
                RtNative.Check(ctx, RtNative.rt_set_option(ctx, "closest_all", countAll ? 1 : 0), "rt_set_option(closest_all)");
                RtNative.Check(ctx, RtNative.rt_closest_points(ctx, points, points.Length, result), "rt_closest_points");
            }
            finally
            {
                RtNative.rt_set_option(ctx, "closest_k", 1);
                RtNative.rt_set_option(ctx, "closest_all", 0);
            }
            return result;
        }

        // how many spheres and triangles lie within tMax of each point: K = 1 with closest_all, the search bounded by the radius alone
        public static unsafe int[] OverlapCount(IntPtr ctx, RtRay[] points)
        {
            var nearest = NearestK(ctx, points, 1, true);
            var counts = new int[nearest.Length];
            fixed (RtClosest* p = nearest)
                for (int i = 0; i < counts.Length; ++i) counts[i] = p[i]._reserved[0];
            return counts;
        }
    }
}
