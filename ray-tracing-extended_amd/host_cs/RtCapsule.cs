// RtCapsule.cs — capsule overlap queries (include/rt.h "capsule overlap queries"): Physics.OverlapCapsule / CheckCapsule over the EXISTING
// imports of RtNative.cs — rt_set_option("closest_capsule", 1), ("closest_k", K) and ("closest_all", 0 / 1), rt_closest_points, and the
// three options back to 0, 1 and 0 in a finally.  No new DllImport and no new record: a capsule is an RtRay (origin = P0, direction =
// P1 - P0, tMax = the radius), the results are RtClosest (RtClosest.cs), K per capsule, capsule-major, nearest to the segment first, the
// unused ones miss records; _reserved[0] of every record of a capsule is the count, _reserved[1] the bits of s, the parameter of the
// segment's closest point.  The options go back to their defaults, not to what they were.
using System;

namespace RtMi355x
{
    public static class RtCapsule
    {
        public const int MaxK = 8;      // RT_HITS_MAX

        // one capsule as the entry takes it: the axis from (ax, ay, az) to (bx, by, bz), d = P1 - P0 formed in float
        public static unsafe RtRay Capsule(float ax, float ay, float az, float bx, float by, float bz, float radius)
        {
            var c = new RtRay();
            c.origin[0] = ax; c.origin[1] = ay; c.origin[2] = az;
            c.tMax = radius;
            c.direction[0] = bx - ax; c.direction[1] = by - ay; c.direction[2] = bz - az;
            return c;
        }

        // countAll: the count is every surface within the radius, not min(found, k)
        public static RtClosest[] OverlapCapsule(IntPtr ctx, RtRay[] capsules, int k = 4, bool countAll = false)
        {
            if (capsules == null) throw new ArgumentNullException(nameof(capsules));
            if (k < 1 || k > MaxK) throw new ArgumentOutOfRangeException(nameof(k), "k: 1..8");
            var result = new RtClosest[capsules.Length * k];
            try
            {
                RtNative.Check(ctx, RtNative.rt_set_option(ctx, "closest_capsule", 1), "rt_set_option(closest_capsule)");
                RtNative.Check(ctx, RtNative.rt_set_option(ctx, "closest_k", k), "rt_set_option(closest_k)");
                RtNative.Check(ctx, RtNative.rt_set_option(ctx, "closest_all", countAll ? 1 : 0), "rt_set_option(closest_all)");
                RtNative.Check(ctx, RtNative.rt_closest_points(ctx, capsules, capsules.Length, result), "rt_closest_points");
            }
            finally
            {
                RtNative.rt_set_option(ctx, "closest_capsule", 0);  // (unchecked: none of them throws, all three are made)
                RtNative.rt_set_option(ctx, "closest_k", 1);
                RtNative.rt_set_option(ctx, "closest_all", 0);
            }
            return result;
        }

        // Physics.CheckCapsule: whether anything lies within the radius of each segment (K = 1: the count is 0 or 1)
        public static unsafe bool[] CheckCapsule(IntPtr ctx, RtRay[] capsules)
        {
            var first = OverlapCapsule(ctx, capsules, 1, false);
            var any = new bool[first.Length];
            fixed (RtClosest* p = first)
                for (int i = 0; i < any.Length; ++i) any[i] = p[i]._reserved[0] != 0;
            return any;
        }
    }
}
