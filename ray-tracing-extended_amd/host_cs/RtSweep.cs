// RtSweep.cs — sphere casts (include/rt.h "sphere casts"): Physics.SphereCast and its yes / no form over the EXISTING imports of
// RtNative.cs — rt_set_option("sweep", 1), rt_trace_rays / rt_occluded, rt_set_option("sweep", 0) in a finally.  No new DllImport.
// Physics.SphereCastAll ("sphere-cast-all") likewise over rt_trace_hits with option "hits_sweep".
// The radius travels as the bits of RtRay._reserved in a copy of the rays; the caller's array is left alone.  The option goes back to
// 0, not to what it was: a caller who has set "sweep" = 1 on the context themselves finds it cleared after either helper.
using System;

namespace RtMi355x
{
    public static class RtSweep
    {
        // RtHit._reserved[0] of a sphere cast: the feature of the contact
        public const int FeatureSphere = 0, FeatureFront = 1, FeatureBack = 2, FeatureEdgeAB = 3, FeatureEdgeAC = 4, FeatureEdgeBC = 5,
                         FeatureVertexA = 6, FeatureVertexB = 7, FeatureVertexC = 8;

        // radii: one value for all rays, or one per ray
        static RtRay[] WithRadius(RtRay[] rays, float[] radii)
        {
            if (rays == null) throw new ArgumentNullException(nameof(rays));
            if (radii == null || (radii.Length != 1 && radii.Length != rays.Length))
                throw new ArgumentException("radii: one value, or one per ray", nameof(radii));
            var copy = (RtRay[])rays.Clone();
            for (int i = 0; i < copy.Length; ++i)
                copy[i]._reserved = BitConverter.ToInt32(BitConverter.GetBytes(radii[radii.Length == 1 ? 0 : i]), 0);  // (every API level has these two)
            return copy;
        }

        // dst = how far the ball travels, hitPoint = the contact, normal = the contact normal, _reserved[0] = the feature
        public static RtHit[] SphereCast(IntPtr ctx, RtRay[] rays, params float[] radii)
        {
            var swept = WithRadius(rays, radii);
            var hits = new RtHit[swept.Length];
            RtNative.Check(ctx, RtNative.rt_set_option(ctx, "sweep", 1), "rt_set_option(sweep)");
            try { RtNative.Check(ctx, RtNative.rt_trace_rays(ctx, swept, swept.Length, hits), "rt_trace_rays"); }
            finally { RtNative.rt_set_option(ctx, "sweep", 0); }
            return hits;
        }

        // 1 where SphereCast would hit
        public static byte[] SphereCheck(IntPtr ctx, RtRay[] rays, params float[] radii)
        {
            var swept = WithRadius(rays, radii);
            var occluded = new byte[swept.Length];
            RtNative.Check(ctx, RtNative.rt_set_option(ctx, "sweep", 1), "rt_set_option(sweep)");
            try { RtNative.Check(ctx, RtNative.rt_occluded(ctx, swept, swept.Length, occluded), "rt_occluded"); }
            finally { RtNative.rt_set_option(ctx, "sweep", 0); }
            return occluded;
        }

        // Physics.SphereCastAll (include/rt.h "sphere-cast-all"): rays.Length * maxHits records, ray-major — the first maxHits (1..8)
        // primitives the ball touches in order of (dst, kind, primitive); side = the side of the face the ball's centre is on,
        // _reserved = the feature, hitCount = min(total, maxHits), or with countAll every primitive touched before tMax.  Over
        // rt_trace_hits with rt_set_option("hits_sweep", 1), put back to 0 in a finally as "sweep" is above.
        public static RtMultiHit[] SphereCastAll(IntPtr ctx, RtRay[] rays, int maxHits, bool countAll, params float[] radii)
        {
            if (maxHits < 1 || maxHits > 8) throw new ArgumentOutOfRangeException(nameof(maxHits), "1..8");
            var swept = WithRadius(rays, radii);
            var hits = new RtMultiHit[swept.Length * maxHits];
            RtHitsParams[] p = { new RtHitsParams { maxHits = maxHits, mode = 0, countAll = countAll ? 1 : 0 } };
            RtNative.Check(ctx, RtNative.rt_set_option(ctx, "hits_sweep", 1), "rt_set_option(hits_sweep)");
            try { RtNative.Check(ctx, RtNative.rt_trace_hits(ctx, swept, swept.Length, p, hits), "rt_trace_hits"); }
            finally { RtNative.rt_set_option(ctx, "hits_sweep", 0); }
            return hits;
        }
    }
}
