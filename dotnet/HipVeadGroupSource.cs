// HipVeadGroupSource.cs — Scylla's read pass behind its own seam: IVeadGroupSource (src/lib/VariantPhasing/Interfaces/IVeadGroupSource.cs),
// made by the virtual Factory.CreateVeadGroupSource (src/lib/VariantPhasing/Factory.cs:124).  The reference's VeadGroupSource reopens the
// BAM for every neighbourhood and walks the chromosome's alignments again; here the chromosome's reads were decoded once onto the device
// (pisces_hip_bam_decode on `handle`) and every neighbourhood is one pisces_hip_vead_groups_device call over them.  The clusterer and
// everything behind it stay managed and unchanged: they get the same VeadGroups in the same order.
// Written against the reference's types; source only (no dotnet toolchain in the build image).
using System;
using System.Collections.Generic;
using System.Runtime.InteropServices;
using Pisces.Domain.Options;
using VariantPhasing.Interfaces;
using VariantPhasing.Models;

namespace Pisces.Hip
{
    public class HipVeadGroupSource : IVeadGroupSource, IDisposable
    {
        // the outputs lie in pinned host memory, which the device writes and the host reads after the stream has drained
        [DllImport("amdhip64", CallingConvention = CallingConvention.Cdecl)] private static extern int hipHostMalloc(out IntPtr ptr, UIntPtr bytes, uint flags);
        [DllImport("amdhip64", CallingConvention = CallingConvention.Cdecl)] private static extern int hipHostFree(IntPtr ptr);
        [DllImport("amdhip64", CallingConvention = CallingConvention.Cdecl)] private static extern int hipStreamSynchronize(IntPtr stream);

        private readonly IntPtr _handle;     // a PiscesHip handle whose decoded batch (pisces_hip_bam_decode) is the chromosome's reads
        private readonly IntPtr _stream;
        private NativeMethods.PiscesVeadOptions _options;
        private IntPtr _groups, _states, _info, _nOut;
        private long _groupCapacity, _stateCapacity;

        public HipVeadGroupSource(IntPtr handle, BamFilterParameters options)
        {
            _handle = handle;
            NativeMethods.Check(IntPtr.Zero, NativeMethods.pisces_hip_vead_default_options(out _options));
            _options.MinBaseCallQuality = options.MinimumBaseCallQuality;
            _options.MinNumberVariantsInRead = options.MinNumberVariantsInRead;
            NativeMethods.Check(handle, NativeMethods.pisces_hip_get_stream(handle, out _stream));
            Pinned(out _info, Marshal.SizeOf<NativeMethods.PiscesVeadNeighborhoodInfo>());
            Pinned(out _nOut, 3 * sizeof(long));
            Reserve(1024, 1024 * 16);
        }

        private static void Pinned(out IntPtr p, long bytes)
        {
            if (hipHostMalloc(out p, (UIntPtr)(ulong)Math.Max(bytes, 1), 0) != 0) throw new Exception("hipHostMalloc failed");
        }

        private void Reserve(long groups, long states)
        {
            if (_groups != IntPtr.Zero) hipHostFree(_groups);
            if (_states != IntPtr.Zero) hipHostFree(_states);
            Pinned(out _groups, groups * Marshal.SizeOf<NativeMethods.PiscesVeadGroup>());
            Pinned(out _states, states);
            _groupCapacity = groups;
            _stateCapacity = states;
        }

        public IEnumerable<VeadGroup> GetVeadGroups(CallableNeighborhood neighborhood)
        {
            var neighbors = neighborhood.VcfVariantSites;   // in the order the reference left them: nothing is sorted here
            var sites = new NativeMethods.PiscesVeadSite[neighbors.Count];
            var alleles = new List<byte>();
            for (var i = 0; i < neighbors.Count; i++)
            {
                var vs = neighbors[i];
                sites[i] = new NativeMethods.PiscesVeadSite { Position = vs.VcfReferencePosition, RefLen = vs.VcfReferenceAllele.Length,
                                                              AltLen = vs.VcfAlternateAllele.Length, AlleleOffset = alleles.Count };
                alleles.AddRange(System.Text.Encoding.ASCII.GetBytes(vs.VcfReferenceAllele));
                alleles.AddRange(System.Text.Encoding.ASCII.GetBytes(vs.VcfAlternateAllele));
            }
            var one = new[] { new NativeMethods.PiscesVeadNeighborhood { SiteBegin = 0, SiteEnd = sites.Length } };
            var bytes = alleles.ToArray();
            long nGroups, nStates;
            while (true)
            {
                var o = new NativeMethods.PiscesVeadOut { Groups = _groups, States = _states, Info = _info, NOut = _nOut,
                                                          GroupCapacity = _groupCapacity, StateCapacity = _stateCapacity };
                NativeMethods.Check(_handle, NativeMethods.pisces_hip_vead_groups_device(_handle, ref _options, IntPtr.Zero, 0, 0, sites, sites.Length, bytes,
                                                                                         bytes.Length, one, 1, ref o, IntPtr.Zero));
                if (hipStreamSynchronize(_stream) != 0) throw new Exception("hipStreamSynchronize failed");
                nGroups = Marshal.ReadInt64(_nOut, 0);
                nStates = Marshal.ReadInt64(_nOut, 8);
                if (nGroups <= _groupCapacity && nStates <= _stateCapacity) break;
                Reserve(Math.Max(nGroups, 2 * _groupCapacity), Math.Max(nStates, 2 * _stateCapacity));   // only the counts were written: repeat
            }
            var info = Marshal.PtrToStructure<NativeMethods.PiscesVeadNeighborhoodInfo>(_info);
            neighborhood.NumberClippedReads += info.NClippedReads;

            var result = new List<VeadGroup>((int)nGroups);
            var size = Marshal.SizeOf<NativeMethods.PiscesVeadGroup>();
            for (long g = 0; g < nGroups; g++)   // in the order of their first read: the order the reference's Dictionary enumerates in
            {
                var native = Marshal.PtrToStructure<NativeMethods.PiscesVeadGroup>(IntPtr.Add(_groups, (int)(g * size)));
                var results = new VariantSite[sites.Length];
                for (var i = 0; i < sites.Length; i++)
                    results[i] = Match(neighbors[i], Marshal.ReadByte(_states, (int)(native.StateOffset + i)));
                var group = new VeadGroup(new Vead("read_" + native.FirstRead, results));
                for (var k = 1; k < native.NVeads; k++) group.AddSupport(group.RepresentativeVead);
                result.Add(group);
            }
            return result;
        }

        // VeadFinder's SetEmptyMatch / SetReferenceMatch / SetVariantMatch / SetDifferenceMatch (VeadFinder.cs:304-334)
        private static VariantSite Match(VariantSite vcfVariant, byte state)
        {
            var m = vcfVariant.DeepCopy();
            switch (state)
            {
                case 1: m.VcfReferenceAllele = vcfVariant.VcfReferenceAllele.Substring(0, 1); m.VcfAlternateAllele = m.VcfReferenceAllele; break;
                case 2: break;
                case 3: m.VcfReferenceAllele = "X"; m.VcfAlternateAllele = "X"; break;
                default: m.VcfReferenceAllele = "N"; m.VcfAlternateAllele = "N"; break;
            }
            return m;
        }

        public void Dispose()
        {
            foreach (var p in new[] { _groups, _states, _info, _nOut })
                if (p != IntPtr.Zero) hipHostFree(p);
            _groups = _states = _info = _nOut = IntPtr.Zero;
        }
    }
}
