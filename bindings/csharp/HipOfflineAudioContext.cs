// HipOfflineAudioContext.cs -- drop-in replacement for OfflineAudioContext (OfflineAudioContext.cs:8-158) that renders
// the graph on an MI355X through libgraphaudio_hip.so.  User code is unchanged: nodes are created against this context,
// connected with AudioNode.Connect, scheduled with Start/Stop and AudioParam automation, then
//     ctx.Render(float[][] output, int frameCount, int startIndex = 0)      // same signature as OfflineAudioContext.cs:30
// Lives INSIDE the GraphAudio.Core assembly (AllowUnsafeBlocks is already on, GraphAudio.Core.csproj:8) because the
// snapshot below reads internal/private state: AudioNode.Params (Nodes/AudioNode.cs:26), AudioParam._events
// (AudioParam.cs:22), AudioBufferSourceNode._startTime/_stopTime/_offset/_duration (AudioBufferSourceNode.cs:19-22),
// AudioNodeInput mode/interpretation (AudioNodeInput.cs:20-21).  INTEGRATION.md lists the five one-line `internal`
// accessors that must be added next to those fields.
//
// Design: the managed side stays the single source of truth for the graph.  Before every Render it (1) drains the
// command queue exactly like AudioContextBase.ProcessBlock does (AudioContextBase.cs:57), (2) walks the graph from
// Destination (same traversal as GetAllNodes, AudioContextBase.cs:191-218), (3) replays what changed since the last
// call through the flat C ABI -- O(graph delta) calls -- and (4) makes ONE ga_render call for the whole frame range.
// Unsupported node types (anything but AudioBufferSourceNode, GainNode, BiQuadFilterNode, ConvolverNode, ChannelSplitterNode,
// ChannelMergerNode, ConstantSourceNode, StereoPannerNode, OscillatorNode, DelayNode, Hip.SpatialPannerNode, Hip.DynamicsCompressorNode and the
// destination) make EnsureSynced throw NotSupportedException; callers fall back to the stock CPU context.
// NOTE: not compiled in this repository's build image (no .NET); reviewed by reading.  The Python host in
// graphaudio_amd/core.py drives the very same C ABI calls in the same order and IS tested.
using System;
using System.Collections.Generic;
using GraphAudio.Nodes;

namespace GraphAudio.Core.Hip;

public sealed unsafe class HipOfflineAudioContext : AudioContextBase
{
    private IntPtr _native;
    private readonly Dictionary<AudioNode, int> _nodeIds = new();
    private readonly Dictionary<PlayableAudioBuffer, int> _bufferIds = new();
    private readonly Dictionary<AudioNode, NodeShadow> _shadow = new();

    public HipOfflineAudioContext(int sampleRate = 48000, int device = 0) : base(sampleRate)
    {
        GraphAudioHip.Check(IntPtr.Zero, GraphAudioHip.ga_context_create(sampleRate, device, out _native));
        _nodeIds[Destination] = 0;
    }

    /// <summary>The native context handle (ga_comm_init and other calls that have no managed wrapper).</summary>
    public IntPtr Handle => _native;

    /// <summary>Render of a voice-sharded graph (INTEGRATION.md section 4): this rank renders its share, the library sums the
    /// destination buses of all ranks with one RCCL reduce; <paramref name="output"/> is written on <paramref name="root"/> only.</summary>
    public void RenderReduce(float[][] output, int frameCount, int startIndex = 0, int root = 0) => RenderCore(output, frameCount, startIndex, root);

    /// <summary>The listener of every SpatialPannerNode of this context: SteamAudioContext.SetListener (SteamAudioContext.cs:145-164)
    /// -- normalise, right = forward x up, ahead = -forward -- stored in the twelve listener_* options of the native context.</summary>
    public void SetListener(System.Numerics.Vector3 position, System.Numerics.Vector3 forward, System.Numerics.Vector3 up)
    {
        var f = System.Numerics.Vector3.Normalize(forward);
        var u = System.Numerics.Vector3.Normalize(up);
        var r = System.Numerics.Vector3.Cross(f, u);
        SetListenerTransform(position, r, u, -f);
    }

    public void SetListenerTransform(System.Numerics.Vector3 origin, System.Numerics.Vector3 right, System.Numerics.Vector3 up, System.Numerics.Vector3 ahead)
    {
        var names = new[] { "origin", "right", "up", "ahead" };
        var vecs = new[] { origin, right, up, ahead };
        for (int v = 0; v < 4; v++)
        {
            GraphAudioHip.Check(_native, GraphAudioHip.ga_set_option(_native, $"listener_{names[v]}_x", vecs[v].X));
            GraphAudioHip.Check(_native, GraphAudioHip.ga_set_option(_native, $"listener_{names[v]}_y", vecs[v].Y));
            GraphAudioHip.Check(_native, GraphAudioHip.ga_set_option(_native, $"listener_{names[v]}_z", vecs[v].Z));
        }
    }

    private bool _spatialParamSignals;
    /// <summary>Option "spatial_param_signals" (default off): signals connected to the AudioParams of a Hip.SpatialPannerNode are
    /// rendered -- the node's per-block descriptors are then made on the device.  Off: such a connection makes Render throw
    /// NotSupportedException before anything moves.  A signal on Occlusion is refused unless SpatialOcclusion is on too.</summary>
    public bool SpatialParamSignals
    {
        get => _spatialParamSignals;
        set
        {
            GraphAudioHip.Check(_native, GraphAudioHip.ga_set_option(_native, "spatial_param_signals", value ? 1 : 0));
            _spatialParamSignals = value;
        }
    }

    private bool _spatialOcclusion;
    /// <summary>Option "spatial_occlusion" (default off): Occlusion above 0 and TransmissionLow / Mid / High of a Hip.SpatialPannerNode
    /// are rendered -- 0 is open air, 1 fully blocked, a transmission the share of its band that passes the obstacle; the stage is
    /// this library's own definition (three bands split at 800 Hz and 8 kHz), not Steam Audio's.  Off: an Occlusion above 0 makes
    /// Render throw NotSupportedException before anything moves.  A signal on Occlusion needs SpatialParamSignals as well.</summary>
    public bool SpatialOcclusion
    {
        get => _spatialOcclusion;
        set
        {
            GraphAudioHip.Check(_native, GraphAudioHip.ga_set_option(_native, "spatial_occlusion", value ? 1 : 0));
            _spatialOcclusion = value;
        }
    }

    private bool _delayFlagExact;
    /// <summary>Option "delay_flag_exact" (default off): the non-silent flag of a DelayNode's output is read from the rendered samples
    /// (the first sample != 0f, as DelayNode.Process raises it) instead of being predicted from the flags of its input blocks.  Costs
    /// one stream wait in the chunks in which a delay's flag may rise; a delay on a feedback loop, behind another undecided delay, behind
    /// a source with a modulated playbackRate or behind a ConvolverNode keeps the prediction (Stats.delay_flags_predicted).</summary>
    public bool DelayFlagExact
    {
        get => _delayFlagExact;
        set
        {
            GraphAudioHip.Check(_native, GraphAudioHip.ga_set_option(_native, "delay_flag_exact", value ? 1 : 0));
            _delayFlagExact = value;
        }
    }

    private bool _convMigrate;
    /// <summary>Option "conv_migrate" (default off): a ConvolverNode that is already running on a fast formulation when an edit makes
    /// it sensitive (its output reaches an AudioParam, a resonant low BiQuadFilterNode or a feedback loop whose gain comes near 1) is
    /// moved to the reference-order formulation.  From the coarse-partition formulation its state is rebuilt from its input history:
    /// from that chunk on its output is what a node on the reference-order formulation from its first block would give, bit for
    /// bit; from a shared-impulse-response group the state is copied and the same holds P blocks later.  One way: the node never
    /// returns to the fast formulation (Stats.conv_migrations counts the nodes moved).</summary>
    public bool ConvMigrate
    {
        get => _convMigrate;
        set
        {
            GraphAudioHip.Check(_native, GraphAudioHip.ga_set_option(_native, "conv_migrate", value ? 1 : 0));
            _convMigrate = value;
        }
    }

    private bool _libmExact;
    /// <summary>Option "libm_exact" (default off): a BiQuadFilterNode or StereoPannerNode whose parameters move computes its
    /// coefficients on the device with cosf / sinf / powf restated from glibc (2.28 and later), so they equal MathF.Cos / Sin / Pow of a
    /// .NET host on glibc bit for bit.  Off: the double-precision functions rounded once, which differ from glibc's in the last bit
    /// for 0.006 % .. 0.09 % of the arguments.  Leave it off where MathF is backed by another C library.</summary>
    public bool LibmExact
    {
        get => _libmExact;
        set
        {
            GraphAudioHip.Check(_native, GraphAudioHip.ga_set_option(_native, "libm_exact", value ? 1 : 0));
            _libmExact = value;
        }
    }

    private bool _spatialBuiltinHrir;
    /// <summary>Option "spatial_builtin_hrir" (default off): a SpatialPannerNode that has no HRIR set of its own renders on the
    /// library's built-in set -- an analytic spherical-head model (Brown and Duda) on a grid of 72 azimuths x 25 elevations, made on the
    /// device at the context's sample rate -- instead of being refused.  A node that has a set keeps it.  The set is this library's own
    /// definition, not Steam Audio's default HRTF (DESIGN.md section 2e, "The built-in set").</summary>
    public bool SpatialBuiltinHrir
    {
        get => _spatialBuiltinHrir;
        set
        {
            GraphAudioHip.Check(_native, GraphAudioHip.ga_set_option(_native, "spatial_builtin_hrir", value ? 1 : 0));
            _spatialBuiltinHrir = value;
        }
    }

    private double _spatialHeadRadius = 0.0875;
    /// <summary>Option "spatial_head_radius": the head radius of the built-in HRIR set in metres, 0.04 .. 0.20 (default 0.0875; outside
    /// the range: ArgumentOutOfRangeException).  A change remakes the set in front of the next block that needs it; nodes on the set
    /// take it up without a crossfade, as after any change of their HRIR set.</summary>
    public double SpatialHeadRadius
    {
        get => _spatialHeadRadius;
        set
        {
            GraphAudioHip.Check(_native, GraphAudioHip.ga_set_option(_native, "spatial_head_radius", value));
            _spatialHeadRadius = value;
        }
    }

    private bool _irResample;
    /// <summary>Option "ir_resample" (default off): ConvolverNode.Buffer and a SpatialPannerNode's HRIR set accept a buffer whose
    /// sample rate is not the context's instead of throwing InvalidOperationException.  The buffer is converted once, when it is
    /// assigned, on the device, by a band-limited (Kaiser-windowed sinc) filter that keeps the response in Hz and the DC gain; the
    /// node works on the converted taps, Normalize included, and an HRIR set's 512-frame limit applies to the converted length.
    /// Rate pairs whose conversion table would exceed 2^22 entries throw NotSupportedException.  The conversion is this library's
    /// own definition (DESIGN.md section 8); turning the option off leaves buffers already assigned alone
    /// (Stats.ir_resamples counts the buffers converted).</summary>
    public bool IrResample
    {
        get => _irResample;
        set
        {
            GraphAudioHip.Check(_native, GraphAudioHip.ga_set_option(_native, "ir_resample", value ? 1 : 0));
            _irResample = value;
        }
    }

    /// <summary>Same contract as OfflineAudioContext.Render (OfflineAudioContext.cs:30-102).</summary>
    public void Render(float[][] output, int frameCount, int startIndex = 0) => RenderCore(output, frameCount, startIndex, -1);

    private void RenderCore(float[][] output, int frameCount, int startIndex, int reduceRoot)
    {
        if (output.Length == 0) throw new ArgumentException("Output buffer must have at least one channel.", nameof(output));
        if (frameCount <= 0) throw new ArgumentOutOfRangeException(nameof(frameCount), "Frame count must be positive.");
        if (startIndex < 0) throw new ArgumentOutOfRangeException(nameof(startIndex), "Start index must be non-negative.");
        for (int ch = 0; ch < output.Length; ch++)
        {
            if (output[ch] is null) throw new ArgumentException($"Channel {ch} buffer is null.", nameof(output));
            if (output[ch].Length < startIndex + frameCount) throw new ArgumentException($"Channel {ch} buffer is too small.", nameof(output));
        }
        EnsureSynced();
        // pin every channel for the duration of the call only (SteamAudioNodeBase.cs:86-95 does the same)
        var handles = new System.Runtime.InteropServices.GCHandle[output.Length];
        float** ptrs = stackalloc float*[output.Length];
        try
        {
            for (int ch = 0; ch < output.Length; ch++)
            {
                handles[ch] = System.Runtime.InteropServices.GCHandle.Alloc(output[ch], System.Runtime.InteropServices.GCHandleType.Pinned);
                ptrs[ch] = (float*)handles[ch].AddrOfPinnedObject();
            }
            GraphAudioHip.Check(_native, reduceRoot < 0
                ? GraphAudioHip.ga_render(_native, ptrs, output.Length, frameCount, startIndex)
                : GraphAudioHip.ga_render_reduce(_native, ptrs, output.Length, frameCount, startIndex, reduceRoot));
        }
        finally
        {
            foreach (var h in handles) if (h.IsAllocated) h.Free();
        }
        RaiseEndedEvents();
    }

    public float[][] Render(int frameCount)   // OfflineAudioContext.cs:108-124
    {
        if (frameCount <= 0) throw new ArgumentOutOfRangeException(nameof(frameCount), "Frame count must be positive.");
        int channels = GraphAudioHip.ga_destination_output_channels(_native);
        var output = new float[channels][];
        for (int ch = 0; ch < channels; ch++) output[ch] = new float[frameCount];
        Render(output, frameCount);
        return output;
    }

    // ---- graph snapshot -> C ABI delta ------------------------------------------------------------------------
    private sealed class NodeShadow
    {
        public List<(AudioNode src, int outIdx)>[] Inputs = Array.Empty<List<(AudioNode, int)>>();
        public int[] ParamVersions = Array.Empty<int>();
        public object? Buffer;
        public int HrirAzimuths = 1;   // SpatialPannerNode: the azimuth count last pushed to the native node
        public bool Started;
    }

    private void EnsureSynced()
    {
        DrainCommandsInternal();                       // internal accessor for DrainCommands (AudioContextBase.cs:272-284)
        foreach (var node in GetAllNodes())            // Destination first, then upstream (AudioContextBase.cs:191-218)
        {
            if (!_nodeIds.TryGetValue(node, out int id)) id = CreateNative(node);
            SyncSettings(node, id);
        }
        foreach (var node in GetAllNodes()) SyncConnections(node, _nodeIds[node]);
    }

    private int CreateNative(AudioNode node)
    {
        // (node type, constructor argument): the argument is the output / input count of a splitter / merger
        // (ChannelSplitterNode.cs:14, ChannelMergerNode.cs:14) or DelayNode's maxDelayTime (DelayNode.cs:22, internal accessor)
        (int type, double arg) = node switch
        {
            AudioBufferSourceNode => (GraphAudioHip.NodeBufferSource, 0.0),
            GainNode => (GraphAudioHip.NodeGain, 0.0),
            BiQuadFilterNode => (GraphAudioHip.NodeBiquad, 0.0),
            ConvolverNode => (GraphAudioHip.NodeConvolver, 0.0),
            ChannelSplitterNode sp => (GraphAudioHip.NodeChannelSplitter, (double)sp.Outputs.Count),
            ChannelMergerNode mg => (GraphAudioHip.NodeChannelMerger, (double)mg.Inputs.Count),
            ConstantSourceNode => (GraphAudioHip.NodeConstantSource, 0.0),
            StereoPannerNode => (GraphAudioHip.NodeStereoPanner, 0.0),
            OscillatorNode => (GraphAudioHip.NodeOscillator, 0.0),
            DelayNode d => (GraphAudioHip.NodeDelay, d.MaxDelayTimeInternal),
            SpatialPannerNode => (GraphAudioHip.NodeSpatialPanner, 0.0),
            DynamicsCompressorNode => (GraphAudioHip.NodeDynamicsCompressor, 0.0),
            _ => throw new NotSupportedException($"{node.GetType().Name} is not on the HIP render path; use OfflineAudioContext"),
        };
        GraphAudioHip.Check(_native, GraphAudioHip.ga_node_create_ex(_native, type, arg, out int id));
        _nodeIds[node] = id;
        _shadow[node] = new NodeShadow();
        return id;
    }

    private int BufferId(PlayableAudioBuffer b)
    {
        if (_bufferIds.TryGetValue(b, out int id)) return id;
        float** ch = stackalloc float*[b.NumberOfChannels];
        var pins = new System.Runtime.InteropServices.GCHandle[b.NumberOfChannels];
        try
        {
            for (int c = 0; c < b.NumberOfChannels; c++)
            {
                pins[c] = System.Runtime.InteropServices.GCHandle.Alloc(b.GetChannelArrayInternal(c), System.Runtime.InteropServices.GCHandleType.Pinned);
                ch[c] = (float*)pins[c].AddrOfPinnedObject();
            }
            GraphAudioHip.Check(_native, GraphAudioHip.ga_buffer_create(_native, ch, b.NumberOfChannels, b.Length, b.SampleRate, out id));
        }
        finally { foreach (var p in pins) if (p.IsAllocated) p.Free(); }
        _bufferIds[b] = id;
        return id;
    }

    private void SyncSettings(AudioNode node, int id)
    {
        var sh = _shadow.TryGetValue(node, out var s) ? s : (_shadow[node] = new NodeShadow());
        // input channel configuration (AudioNodeInput.cs:41-58): cheap, always replayed
        for (int i = 0; i < node.Inputs.Count; i++)
        {
            var inp = node.Inputs[i];
            GraphAudioHip.Check(_native, GraphAudioHip.ga_input_set_channel_count(_native, id, i, inp.ChannelCount));
            GraphAudioHip.Check(_native, GraphAudioHip.ga_input_set_channel_count_mode(_native, id, i, (int)inp.ChannelCountModeInternal));
        }
        // params: value + event list replayed when the copy-on-write array changed (AudioParam.cs:333-352)
        var ps = node.Params;
        if (sh.ParamVersions.Length != ps.Count) sh.ParamVersions = new int[ps.Count];
        for (int p = 0; p < ps.Count; p++)
        {
            var ev = ps[p].EventsInternal;              // AutomationEvent[] snapshot
            int version = HashCode.Combine(ev, ps[p].Value);
            if (version == sh.ParamVersions[p]) continue;
            sh.ParamVersions[p] = version;
            GraphAudioHip.Check(_native, GraphAudioHip.ga_param_set_value(_native, id, p, ps[p].Value));   // also clears native events
            foreach (var e in ev)
            {
                int rc = e.Type switch
                {
                    0 => GraphAudioHip.ga_param_set_value_at_time(_native, id, p, e.Value, e.Time),
                    1 => GraphAudioHip.ga_param_linear_ramp_to_value_at_time(_native, id, p, e.Value, e.Time),
                    2 => GraphAudioHip.ga_param_exponential_ramp_to_value_at_time(_native, id, p, e.Value, e.Time),
                    _ => GraphAudioHip.ga_param_set_target_at_time(_native, id, p, e.Target, e.Time, e.TimeConstant),
                };
                GraphAudioHip.Check(_native, rc);
            }
        }
        switch (node)
        {
            case BiQuadFilterNode bq:
                GraphAudioHip.Check(_native, GraphAudioHip.ga_biquad_set_type(_native, id, (int)bq.Type));
                break;
            case ConvolverNode cv when !ReferenceEquals(sh.Buffer, cv.Buffer):
                GraphAudioHip.Check(_native, GraphAudioHip.ga_convolver_set_normalize(_native, id, cv.Normalize ? 1 : 0));
                GraphAudioHip.Check(_native, GraphAudioHip.ga_convolver_set_enable_true_stereo(_native, id, cv.EnableTrueStereo ? 1 : 0));
                GraphAudioHip.Check(_native, GraphAudioHip.ga_convolver_set_buffer(_native, id, cv.Buffer is null ? -1 : BufferId(cv.Buffer)));
                sh.Buffer = cv.Buffer;
                break;
            case SpatialPannerNode sp:
                GraphAudioHip.Check(_native, GraphAudioHip.ga_param_set_value(_native, id, GraphAudioHip.SpatialDistanceModel, (int)sp.DistanceModel));
                if (!ReferenceEquals(sh.Buffer, sp.Hrir) || sh.HrirAzimuths != sp.HrirAzimuths)
                {
                    // azimuth count first: the set's channel count is checked against it (graphaudio_hip.h, ga_convolver_set_buffer)
                    GraphAudioHip.Check(_native, GraphAudioHip.ga_convolver_set_buffer(_native, id, -1));
                    GraphAudioHip.Check(_native, GraphAudioHip.ga_param_set_value(_native, id, GraphAudioHip.SpatialHrirAzimuths, sp.HrirAzimuths));
                    GraphAudioHip.Check(_native, GraphAudioHip.ga_convolver_set_buffer(_native, id, sp.Hrir is null ? -1 : BufferId(sp.Hrir)));
                    sh.Buffer = sp.Hrir;
                    sh.HrirAzimuths = sp.HrirAzimuths;
                }
                break;
            case OscillatorNode osc:
                GraphAudioHip.Check(_native, GraphAudioHip.ga_oscillator_set_type(_native, id, (int)osc.Type));
                SyncScheduled(osc, id, sh);
                break;
            case ConstantSourceNode cs:
                SyncScheduled(cs, id, sh);
                break;
            case AudioBufferSourceNode src:
                if (!ReferenceEquals(sh.Buffer, src.Buffer))
                {
                    GraphAudioHip.Check(_native, GraphAudioHip.ga_source_set_buffer(_native, id, src.Buffer is null ? -1 : BufferId(src.Buffer)));
                    sh.Buffer = src.Buffer;
                }
                GraphAudioHip.Check(_native, GraphAudioHip.ga_source_set_loop(_native, id, src.Loop ? 1 : 0, src.LoopStart, src.LoopEnd));
                if (src.HasStartedInternal && !sh.Started)
                {
                    GraphAudioHip.Check(_native, GraphAudioHip.ga_source_start(_native, id, src.StartTimeInternal, src.OffsetInternal, src.DurationInternal));
                    sh.Started = true;
                }
                if (!double.IsNaN(src.StopTimeInternal) && double.IsPositiveInfinity(src.DurationInternal))
                    GraphAudioHip.Check(_native, GraphAudioHip.ga_source_stop(_native, id, src.StopTimeInternal));
                break;
        }
    }

    // Start / Stop of ConstantSourceNode and OscillatorNode (IAudioScheduledSourceNode): NaN duration = none
    private void SyncScheduled(IAudioScheduledSourceNode src, int id, NodeShadow sh)
    {
        if (src.HasStartedInternal && !sh.Started)
        {
            GraphAudioHip.Check(_native, GraphAudioHip.ga_source_start(_native, id, src.StartTimeInternal, 0.0, double.NaN));
            sh.Started = true;
        }
        if (!double.IsNaN(src.StopTimeInternal))
            GraphAudioHip.Check(_native, GraphAudioHip.ga_source_stop(_native, id, src.StopTimeInternal));
    }

    private void SyncConnections(AudioNode node, int id)
    {
        var sh = _shadow.TryGetValue(node, out var s) ? s : (_shadow[node] = new NodeShadow());
        if (sh.Inputs.Length != node.Inputs.Count)
        {
            sh.Inputs = new List<(AudioNode, int)>[node.Inputs.Count];
            for (int i = 0; i < sh.Inputs.Length; i++) sh.Inputs[i] = new();
        }
        for (int i = 0; i < node.Inputs.Count; i++)
        {
            var now = new List<(AudioNode, int)>();
            foreach (var o in node.Inputs[i].ConnectedOutputs) now.Add((o.Owner, o.Index));
            var before = sh.Inputs[i];
            bool same = before.Count == now.Count;
            for (int k = 0; same && k < now.Count; k++) same = ReferenceEquals(before[k].src, now[k].Item1) && before[k].outIdx == now[k].Item2;
            if (same) continue;
            // connection ORDER is semantic (sequential float32 sum, AudioNodeInput.cs:121-132): rebuild the list in order
            foreach (var (src, outIdx) in before) GraphAudioHip.Check(_native, GraphAudioHip.ga_node_disconnect(_native, _nodeIds[src], id, outIdx, i));
            foreach (var (src, outIdx) in now) GraphAudioHip.Check(_native, GraphAudioHip.ga_node_connect(_native, _nodeIds[src], id, outIdx, i));
            sh.Inputs[i] = now;
        }
    }

    private void RaiseEndedEvents()
    {
        foreach (var (node, id) in _nodeIds)
            if (node is AudioBufferSourceNode src && GraphAudioHip.ga_node_has_ended(_native, id) == 1)
                src.RaiseEndedFromNative();            // raises Ended once and Dispose()s, like TryRaiseEndedEvent (:378-389)
    }

    protected override void Dispose(bool disposing)
    {
        if (_native != IntPtr.Zero)
        {
            GraphAudioHip.ga_context_destroy(_native);
            _native = IntPtr.Zero;
        }
        base.Dispose(disposing);
    }
}

/// <summary>
/// The parameter surface of GraphAudio.SteamAudio's SpatialPannerNode (SpatialPannerNode.cs:17-47,94-114) without its Steam Audio
/// dependency: a node of this type exists to be rendered by HipOfflineAudioContext, which runs the binaural stage on the HRIR set
/// assigned here (DESIGN.md "SpatialPannerNode").  A Kit Sound that targets the HIP path creates this node instead (INTEGRATION.md).
/// </summary>
public sealed class SpatialPannerNode : AudioNode
{
    public enum DistanceModelType { Linear, Inverse, Exponential }

    // (name, default, min, max) in the native parameter order; all k-rate
    private static readonly (string name, float def, float min, float max)[] Table =
    {
        ("positionX", 0f, float.MinValue, float.MaxValue), ("positionY", 0f, float.MinValue, float.MaxValue), ("positionZ", 0f, float.MinValue, float.MaxValue),
        ("orientationX", 1f, -1f, 1f), ("orientationY", 0f, -1f, 1f), ("orientationZ", 0f, -1f, 1f),
        ("refDistance", 1f, 0f, float.MaxValue), ("maxDistance", 10000f, 0f, float.MaxValue), ("rolloffFactor", 1f, 0f, float.MaxValue),
        ("coneInnerAngle", 360f, 0f, 360f), ("coneOuterAngle", 360f, 0f, 360f), ("coneOuterGain", 0f, 0f, 1f),
        ("spatialBlend", 1f, 0f, 1f), ("occlusion", 0f, 0f, 1f),
        ("transmissionLow", 0f, 0f, 1f), ("transmissionMid", 0f, 0f, 1f), ("transmissionHigh", 0f, 0f, 1f),
    };
    private readonly AudioParam[] _p = new AudioParam[Table.Length];

    public AudioParam PositionX => _p[0]; public AudioParam PositionY => _p[1]; public AudioParam PositionZ => _p[2];
    public AudioParam OrientationX => _p[3]; public AudioParam OrientationY => _p[4]; public AudioParam OrientationZ => _p[5];
    public AudioParam RefDistance => _p[6]; public AudioParam MaxDistance => _p[7]; public AudioParam RolloffFactor => _p[8];
    public AudioParam ConeInnerAngle => _p[9]; public AudioParam ConeOuterAngle => _p[10]; public AudioParam ConeOuterGain => _p[11];
    public AudioParam SpatialBlend => _p[12]; public AudioParam Occlusion => _p[13];
    public AudioParam TransmissionLow => _p[14]; public AudioParam TransmissionMid => _p[15]; public AudioParam TransmissionHigh => _p[16];

    public DistanceModelType DistanceModel { get; set; } = DistanceModelType.Inverse;
    /// <summary>2 * D channels x T frames (T at most 512): channel 2d = left ear, 2d + 1 = right ear of direction d = j * HrirAzimuths + i.</summary>
    public PlayableAudioBuffer? Hrir { get; set; }
    public int HrirAzimuths { get; set; } = 1;

    public SpatialPannerNode(HipOfflineAudioContext context) : base(context, inputCount: 1, outputCount: 1, "SpatialPanner")
    {
        for (int i = 0; i < Table.Length; i++) _p[i] = CreateAudioParam(Table[i].name, Table[i].def, Table[i].min, Table[i].max, AutomationRate.KRate);
        Inputs[0].SetChannelCount(2);
        Inputs[0].SetChannelCountMode(ChannelCountMode.ClampedMax);
        Inputs[0].SetChannelInterpretation(ChannelInterpretation.Speakers);
    }

    protected override void Process() => throw new NotSupportedException("SpatialPannerNode (HIP) is rendered by HipOfflineAudioContext only");
}

/// <summary>
/// A bus compressor / limiter rendered by HipOfflineAudioContext (native node type 13): the library's own definition
/// (include/graphaudio_hip.h, DESIGN.md section 2g) -- GraphAudio.Core has no such node, so the stock CPU context cannot render it.
/// One input (2 channels, clamped-max, speakers), one output with the input's channel count; all parameters k-rate.  Connecting a
/// signal to a parameter makes the native library answer GA_ERR_UNSUPPORTED (NotSupportedException from EnsureSynced).
/// </summary>
public sealed class DynamicsCompressorNode : AudioNode
{
    // (name, default, min, max) in the native parameter order
    private static readonly (string name, float def, float min, float max)[] Table =
    {
        ("threshold", -24f, -100f, 0f), ("knee", 30f, 0f, 40f), ("ratio", 12f, 1f, 20f),
        ("attack", 0.003f, 0f, 1f), ("release", 0.25f, 0f, 1f), ("makeupGain", 0f, -40f, 40f),
    };
    private readonly AudioParam[] _p = new AudioParam[Table.Length];

    public AudioParam Threshold => _p[0]; public AudioParam Knee => _p[1]; public AudioParam Ratio => _p[2];
    public AudioParam Attack => _p[3]; public AudioParam Release => _p[4]; public AudioParam MakeupGain => _p[5];

    public DynamicsCompressorNode(HipOfflineAudioContext context) : base(context, inputCount: 1, outputCount: 1, "DynamicsCompressor")
    {
        for (int i = 0; i < Table.Length; i++) _p[i] = CreateAudioParam(Table[i].name, Table[i].def, Table[i].min, Table[i].max, AutomationRate.KRate);
        Inputs[0].SetChannelCount(2);
        Inputs[0].SetChannelCountMode(ChannelCountMode.ClampedMax);
        Inputs[0].SetChannelInterpretation(ChannelInterpretation.Speakers);
    }

    protected override void Process() => throw new NotSupportedException("DynamicsCompressorNode (HIP) is rendered by HipOfflineAudioContext only");
}
