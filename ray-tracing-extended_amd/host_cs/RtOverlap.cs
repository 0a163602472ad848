// RtOverlap.cs — box overlap queries (include/rt.h "box overlap queries"): Physics.OverlapBox / CheckBox over the EXISTING imports of
// RtNative.cs — rt_set_option("closest_box", 1), ("closest_k", K) and ("closest_all", 0 / 1), rt_closest_points, and the three options
// back to 0, 1 and 0 in a finally.  No new DllImport and no new record: a box is an RtRay (origin = centre, direction = half-extents,
// tMax > 0 only a gate), the results are RtClosest (RtClosest.cs), K per box, box-major, nearest to the centre first, the unused ones
// miss records; _reserved[0] of every record of a box is the count.  The options go back to their defaults, not to what they were.
using System;

namespace RtMi355x
{
    public static class RtOverlap
    {
        public const int MaxK = 8;      // RT_HITS_MAX

        // one box as the entry takes it
        public static unsafe RtRay Box(float cx, float cy, float cz, float hx, float hy, float hz)
        {
            var b = new RtRay();
            b.origin[0] = cx; b.origin[1] = cy; b.origin[2] = cz;
            b.tMax = 1.0f;
            b.direction[0] = hx; b.direction[1] = hy; b.direction[2] = hz;
            return b;
        }

        // countAll: the count is every surface that touches the box, not min(found, k)
        public static RtClosest[] OverlapBox(IntPtr ctx, RtRay[] boxes, int k = 4, bool countAll = false)
        {
            if (boxes == null) throw new ArgumentNullException(nameof(boxes));
            if (k < 1 || k > MaxK) throw new ArgumentOutOfRangeException(nameof(k), "k: 1..8");
            var result = new RtClosest[boxes.Length * k];
            try
            {
                RtNative.Check(ctx, RtNative.rt_set_option(ctx, "closest_box", 1), "rt_set_option(closest_box)");
                RtNative.Check(ctx, RtNative.rt_set_option(ctx, "closest_k", k), "rt_set_option(closest_k)");
                RtNative.Check(ctx, RtNative.rt_set_option(ctx, "closest_all", countAll ? 1 : 0), "rt_set_option(closest_all)");
                RtNative.Check(ctx, RtNative.rt_closest_points(ctx, boxes, boxes.Length, result), "rt_closest_points");
            }
            finally
            {
                RtNative.rt_set_option(ctx, "closest_box", 0);      // (unchecked: none of them throws, all three are made)
                RtNative.rt_set_option(ctx, "closest_k", 1);
                RtNative.rt_set_option(ctx, "closest_all", 0);
            }
            return result;
        }

        // Physics.CheckBox: whether anything touches each box (K = 1: the count is 0 or 1)
        public static unsafe bool[] CheckBox(IntPtr ctx, RtRay[] boxes)
        {
            var first = OverlapBox(ctx, boxes, 1, false);
            var any = new bool[first.Length];
            fixed (RtClosest* p = first)
                for (int i = 0; i < any.Length; ++i) any[i] = p[i]._reserved[0] != 0;
            return any;
        }
    }
}
