// HipNeighborhoodBuilder.cs — Scylla's neighbourhood builder behind its own seam: INeighborhoodBuilder
// (src/lib/VariantPhasing/Interfaces/INeighborhoodBuilder.cs), made by the virtual Factory.CreateNeighborhoodBuilder.  The reference's
// NeighborhoodBuilder reads the input VCF line by line; here the chromosome's called rows lie on the device where a flush left them
// (`rows`, device pointers) and ONE pisces_hip_nbhd_build_device call answers which of them chain into which neighbourhood.  `alleles`
// are the same rows as managed CalledAlleles, in the same order: the shim only needs them to hand Scylla its own objects back.
// The tables land in pinned host memory, so the sites, allele bytes and neighbourhoods can go to pisces_hip_vead_groups_device as they
// are (HipVeadGroupSource).  Every neighbourhood comes out of the first call; the call after it reports none, which ends VariantPhaser's
// loop.  The VcfNeighborhood is filled in the PRE-sort order (site_original) and CallableNeighborhood's constructor orders it and sets
// the range as it always does; the library's own order (site_row) is List.Sort's up to 16 sites and the stable one above (DESIGN section 7).
// Written against the reference's types; source only (no dotnet toolchain in the build image).
using System;
using System.Collections.Generic;
using System.Runtime.InteropServices;
using Pisces.Domain.Models;
using Pisces.Domain.Models.Alleles;
using Pisces.Domain.Options;
using VariantPhasing.Interfaces;
using VariantPhasing.Models;

namespace Pisces.Hip
{
    public class HipNeighborhoodBuilder : INeighborhoodBuilder, IDisposable
    {
        [DllImport("amdhip64", CallingConvention = CallingConvention.Cdecl)] private static extern int hipHostMalloc(out IntPtr ptr, UIntPtr bytes, uint flags);
        [DllImport("amdhip64", CallingConvention = CallingConvention.Cdecl)] private static extern int hipHostFree(IntPtr ptr);
        [DllImport("amdhip64", CallingConvention = CallingConvention.Cdecl)] private static extern int hipStreamSynchronize(IntPtr stream);

        private readonly IntPtr _handle, _stream;
        private readonly NativeMethods.PiscesVennRows _rows;
        private readonly IReadOnlyList<CalledAllele> _alleles;
        private readonly VariantCallingParameters _variantCallingParams;
        private readonly ChrReference _chrReference;
        private NativeMethods.PiscesNbhdCriteria _criteria;
        private NativeMethods.PiscesNbhdOut _out;
        private bool _done;

        public HipNeighborhoodBuilder(IntPtr handle, PhasableVariantCriteria criteria, VariantCallingParameters variantCallingParams,
                                      NativeMethods.PiscesVennRows rows, IReadOnlyList<CalledAllele> alleles, ChrReference chrReference = null)
        {
            _handle = handle;
            _rows = rows;
            _alleles = alleles;
            _variantCallingParams = variantCallingParams;
            _chrReference = chrReference;
            NativeMethods.Check(IntPtr.Zero, NativeMethods.pisces_hip_nbhd_default_criteria(out _criteria));
            _criteria.PhasingDistance = criteria.PhasingDistance;
            _criteria.PassingVariantsOnly = criteria.PassingVariantsOnly ? 1 : 0;
            _criteria.HetVariantsOnly = criteria.HetVariantsOnly ? 1 : 0;
            _criteria.MinPassingVariantsInNbhd = criteria.MinPassingVariantsInNbhd;
            NativeMethods.Check(handle, NativeMethods.pisces_hip_get_stream(handle, out _stream));
            Pinned(out _out.NOut, 6 * sizeof(long));
        }

        private static void Pinned(out IntPtr p, long bytes)
        {
            if (hipHostMalloc(out p, (UIntPtr)(ulong)Math.Max(bytes, 1), 0) != 0) throw new Exception("hipHostMalloc failed");
        }

        private void Reserve(long nbhds, long sites, long alleleBytes, long refBytes)
        {
            Release(keepCounts: true);
            Pinned(out _out.Sites, sites * Marshal.SizeOf<NativeMethods.PiscesVeadSite>());
            Pinned(out _out.Alleles, alleleBytes);
            Pinned(out _out.SiteRow, sites * sizeof(int));
            Pinned(out _out.SiteOriginal, sites * sizeof(int));
            Pinned(out _out.Neighbourhoods, nbhds * Marshal.SizeOf<NativeMethods.PiscesVeadNeighborhood>());
            Pinned(out _out.Info, nbhds * Marshal.SizeOf<NativeMethods.PiscesNbhdInfo>());
            Pinned(out _out.RefBytes, refBytes);
            _out.NbhdCapacity = nbhds; _out.SiteCapacity = sites; _out.AlleleCapacity = alleleBytes; _out.RefCapacity = refBytes;
        }

        /// <summary>The tables of the last build, for the read pass: pinned host memory the device can read.</summary>
        public NativeMethods.PiscesNbhdOut Tables => _out;

        public IEnumerable<CallableNeighborhood> GetBatchOfCallableNeighborhoods(int numSoFar, out int rawNumNeighborhoods)
        {
            rawNumNeighborhoods = 0;
            var result = new List<CallableNeighborhood>();
            if (_done) return result;
            _done = true;
            var counts = new long[6];
            while (true)   // counts first; when one is above its capacity only the counts were written: repeat with larger arrays
            {
                var rows = _rows;
                NativeMethods.Check(_handle, NativeMethods.pisces_hip_nbhd_build_device(_handle, ref _criteria, ref rows, ref _out, IntPtr.Zero));
                if (hipStreamSynchronize(_stream) != 0) throw new Exception("hipStreamSynchronize failed");
                Marshal.Copy(_out.NOut, counts, 0, 6);
                if (counts[0] < 0)
                    throw new ArgumentException(counts[1] == 0 ? "the rows are not sorted by position at row " + counts[2]
                                                               : "row " + counts[2] + " has no candidate to take its alleles from");
                if (counts[0] <= _out.NbhdCapacity && counts[1] <= _out.SiteCapacity && counts[2] <= _out.AlleleCapacity && counts[3] <= _out.RefCapacity) break;
                Reserve(counts[0], counts[1], counts[2], counts[3]);
            }
            rawNumNeighborhoods = (int)counts[4];
            var infoSize = Marshal.SizeOf<NativeMethods.PiscesNbhdInfo>();
            for (long k = 0; k < counts[0]; k++)
            {
                var info = Marshal.PtrToStructure<NativeMethods.PiscesNbhdInfo>(IntPtr.Add(_out.Info, (int)(k * infoSize)));
                var begin = Marshal.ReadInt32(_out.Neighbourhoods, (int)(k * 8));
                var end = Marshal.ReadInt32(_out.Neighbourhoods, (int)(k * 8 + 4));
                // the sites as NeighborhoodBuilder appended them: site_original is the pre-sort order
                VariantSite Site(int s) => new VariantSite(_alleles[Marshal.ReadInt32(_out.SiteOriginal, s * sizeof(int))]);
                var first = Site(begin);
                var nbhd = new VcfNeighborhood(numSoFar + info.RawIndex, first.ReferenceName, first, Site(begin + 1));
                for (var s = begin + 2; s < end; s++) nbhd.AddVariantSite(Site(s));
                result.Add(new CallableNeighborhood(nbhd, _variantCallingParams, _chrReference));   // orders the sites and sets the range
            }
            return result;
        }

        private void Release(bool keepCounts)
        {
            foreach (var p in new[] { _out.Sites, _out.Alleles, _out.SiteRow, _out.SiteOriginal, _out.Neighbourhoods, _out.Info, _out.RefBytes })
                if (p != IntPtr.Zero) hipHostFree(p);
            _out.Sites = _out.Alleles = _out.SiteRow = _out.SiteOriginal = _out.Neighbourhoods = _out.Info = _out.RefBytes = IntPtr.Zero;
            if (!keepCounts && _out.NOut != IntPtr.Zero) { hipHostFree(_out.NOut); _out.NOut = IntPtr.Zero; }
        }

        public void Dispose() => Release(keepCounts: false);
    }
}
