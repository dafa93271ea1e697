/*
 * aptgpu_decode.c — minimal C caller of the drop-in boundary (include/aptgpu.h):
 *
 *     aptgpu_decode in.wav out.pgm [contrast: telemetry|percent|minmax] [--no-sync]
 *                   [--histogram | --histogram-float] [--palette FILE] [--lab] [--map SHAPEFILE_DIR --track FILE [--fit]] [--png]
 *                   [--tle FILE --sat NAME (--start-ms N | --end-ms N)] [--rotate no|yes|orbit]
 *                   [--project equirect|mercator[:step_deg] [--grid DEG]] [--despeckle R[:T]] [--track=[W,LAMBDA[,LAG]]]
 *                   [--live SECONDS] [--iq FMT:FS:D[:SHIFT_HZ]] [--sun A|B:UNIX_MS[:BLACK] --track FILE]
 *                   [--land-mask SHAPEFILE_DIR --track FILE]
 *
 * What `noaa-apt in.wav -o out.png` does (main.rs:91-110, noaa_apt.rs:114-235): load -> decode ->
 * contrast limits -> 8-bit image, written as a binary PGM, or with --png as the PNG file the GPU
 * encodes (aptgpu_process_image_png: gray, or RGBA with --palette / --map; only the file's bytes
 * cross to the host).  --histogram: Contrast::Histogram (MinMax limits, then each channel's histogram
 * equalised).  --histogram-float: APTGPU_CONTRAST_HISTOGRAM_FLOAT, the equalisation on the f32 samples before they
 * become 8-bit pixels (gray only: refused with --palette).  --palette FILE: false colour (`-F`, tune values 0) from a raw 256 x 256 RGB palette
 * (196 608 bytes, pixel (a, b) at (b*256 + a)*3), written as a binary PPM (the RGBA image without
 * its alpha).  --lab: with --histogram and --palette, equalise the false-colour image as the
 * reference does, channel A in CIE Lab (APTGPU_COLOR_EQUALIZE_LAB); without it that combination
 * is refused.  --map DIR --track FILE: the map overlay (`--map`) of DIR/states.shp, countries.shp and
 * lakes.shp with the default settings and colours; FILE holds the satellite's raw f64 (lat, lon)
 * pairs in radians, one per image row (SGP4 is the caller's job); written as a PPM.  With --fit the overlay's yaw,
 * hscale and vscale and the pass's time offset are fitted to the image first (aptgpu_fit_overlay with its default
 * settings, printed): FILE then holds 120 more rows at either end, image row 0 being its row 120.
 * --project KIND[:STEP]: the finished image (channel A) reprojected onto a north-up equirectangular or
 * Mercator grid of STEP degrees per pixel (default 0.04) that aptgpu_projection_fit sizes from the track
 * (--track FILE, or --tle: aptgpu_sat_track_host), bilinear; --grid DEG adds a graticule.  Written as a
 * PPM of the grid's size, or with --png as the RGBA PNG (transparent off the swath).
 * --despeckle R[:T]: the decoded rows go through aptgpu_despeckle first, a (2R+1) x (2R+1) median (R = 1 or 2) that
 * never leaves a pixel's column band; T (default 0) is the fraction of the 98 % range a sample must differ from the
 * median by to be replaced.
 * --track=W,LAMBDA (or --track= for the defaults 8,0.1; with the equals sign: --track FILE is the satellite's track):
 * the rows come from aptgpu_decode_tracked, the flywheel sync stage in place of find_sync — row starts tracked through
 * noise and dropouts, W work samples of jitter per row at LAMBDA per sample; it also decodes what the plain decode
 * refuses as "less than 5 sync frames".
 * --live SECONDS --track=W,LAMBDA[,LAG] together: a live-decode stream whose rows the flywheel tracker finds, committed LAG
 * rows (default 8) behind the best survivor (aptgpu_stream_create_tracked; with --iq: aptgpu_iq_live_create_tracked).  LAG
 * without --live, and --iq with --track= without --live, are refused.
 * --live SECONDS: the recording goes through a live-decode stream (aptgpu_stream_*) in chunks of SECONDS, as a ground
 * station would feed it during the pass; every push hands back the rows that are final, and their concatenation — the
 * image written — is the same PGM as without the flag.
 * --iq FMT:FS:D[:SHIFT_HZ]: the input file is raw interleaved IQ (FMT u8, s8, s16 or f32; FS frames per second; the
 * audio comes out at FS / D; the signal sits SHIFT_HZ off the centre) with the library's usual channel filter.  Without
 * --live the frames go through aptgpu_fm_demodulate and aptgpu_decode; with --live SECONDS through aptgpu_iq_live_* in
 * chunks of SECONDS of frames, the audio never leaving the device.  Both write the same PGM.
 * --afc[=MAX_HZ] (with --iq, without --live): the carrier is followed block by block and the frames go through
 * aptgpu_fm_demodulate_afc instead: for a recording whose SHIFT_HZ is known only to within MAX_HZ (default 15000), the
 * tuner's error and the Doppler shift of the pass.  The carrier's offset at the start, the middle and the end is printed.
 * --sun A|B:UNIX_MS[:BLACK] --track FILE: the rows go through aptgpu_geolocate first, which divides channel A's or B's
 * video by the cosine of the solar zenith angle at every pixel (capped at 80 degrees), for a pass that starts at
 * UNIX_MS; BLACK is the zero level in row units (default: wedge 9 of the telemetry, the zero-modulation wedge).
 * --land-mask DIR --track FILE: instead of the image, the land / sea / lake mask of the swath (aptgpu_land_mask) from
 * DIR/countries.shp and DIR/lakes.shp, as a 909-wide PGM of the classes 0 sea, 1 land, 2 lake, 255 invalid.
 * Plain C99, links only libaptgpu.so.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aptgpu.h"

static void on_status(float progress, const char *text, void *user)
{
    (void)user;
    fprintf(stderr, "[%3.0f%%] %s\n", progress * 100.f, text);
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        fprintf(stderr, "usage: %s in.wav out.pgm [telemetry|percent|minmax] [--no-sync] [--histogram | --histogram-float] "
                "[--palette FILE] [--lab] [--map SHAPEFILE_DIR --track FILE [--fit]] [--png]\n"
                "       [--tle FILE --sat NAME (--start-ms N | --end-ms N)] [--rotate no|yes|orbit]\n"
                "       [--project equirect|mercator[:step_deg] [--grid DEG]] [--despeckle R[:T]] [--track=[W,LAMBDA[,LAG]]]\n"
                "       [--live SECONDS] [--iq u8|s8|s16|f32:FS:D[:SHIFT_HZ] [--afc[=MAX_HZ]]] [--sun A|B:UNIX_MS[:BLACK] --track FILE]\n"
                "       [--land-mask SHAPEFILE_DIR --track FILE]\n", argv[0]);
        return 2;
    }
    int contrast = APTGPU_CONTRAST_PERCENT, sync = 1, lab = 0, png = 0, fit = 0;
    const char *palette_path = NULL, *map_dir = NULL, *track_path = NULL, *tle_path = NULL, *sat = NULL;
    int rotate = APTGPU_ROTATE_NO, ref_kind = -1;
    long long ref_ms = 0;
    const char *project = NULL, *despeckle = NULL, *flywheel = NULL, *iq_spec = NULL, *sun = NULL, *land_dir = NULL;
    double grid_deg = 0.0, live_seconds = 0.0, afc_max_hz = 15000.0;
    int afc = 0;
    for (int i = 3; i < argc; ++i) {
        if (!strcmp(argv[i], "telemetry")) contrast = APTGPU_CONTRAST_TELEMETRY;
        else if (!strcmp(argv[i], "percent")) contrast = APTGPU_CONTRAST_PERCENT;
        else if (!strcmp(argv[i], "minmax")) contrast = APTGPU_CONTRAST_MINMAX;
        else if (!strcmp(argv[i], "--histogram")) contrast = APTGPU_CONTRAST_HISTOGRAM;
        else if (!strcmp(argv[i], "--histogram-float")) contrast = APTGPU_CONTRAST_HISTOGRAM_FLOAT;
        else if (!strcmp(argv[i], "--no-sync")) sync = 0;
        else if (!strcmp(argv[i], "--lab")) lab = 1;
        else if (!strcmp(argv[i], "--png")) png = 1;
        else if (!strcmp(argv[i], "--fit")) fit = 1;
        else if (!strcmp(argv[i], "--palette") && i + 1 < argc) palette_path = argv[++i];
        else if (!strcmp(argv[i], "--map") && i + 1 < argc) map_dir = argv[++i];
        else if (!strcmp(argv[i], "--track") && i + 1 < argc) track_path = argv[++i];
        else if (!strncmp(argv[i], "--track=", 8)) flywheel = argv[i] + 8;
        else if (!strcmp(argv[i], "--tle") && i + 1 < argc) tle_path = argv[++i];
        else if (!strcmp(argv[i], "--sat") && i + 1 < argc) sat = argv[++i];
        else if (!strcmp(argv[i], "--start-ms") && i + 1 < argc) ref_kind = APTGPU_REF_TIME_START, ref_ms = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--end-ms") && i + 1 < argc) ref_kind = APTGPU_REF_TIME_END, ref_ms = atoll(argv[++i]);
        else if (!strcmp(argv[i], "--project") && i + 1 < argc) project = argv[++i];
        else if (!strcmp(argv[i], "--grid") && i + 1 < argc) grid_deg = atof(argv[++i]);
        else if (!strcmp(argv[i], "--despeckle") && i + 1 < argc) despeckle = argv[++i];
        else if (!strcmp(argv[i], "--live") && i + 1 < argc) live_seconds = atof(argv[++i]);
        else if (!strcmp(argv[i], "--iq") && i + 1 < argc) iq_spec = argv[++i];
        else if (!strcmp(argv[i], "--sun") && i + 1 < argc) sun = argv[++i];
        else if (!strcmp(argv[i], "--land-mask") && i + 1 < argc) land_dir = argv[++i];
        else if (!strcmp(argv[i], "--afc")) afc = 1;
        else if (!strncmp(argv[i], "--afc=", 6)) afc = 1, afc_max_hz = atof(argv[i] + 6); /* (0 or no number: refused by the library) */
        else if (!strcmp(argv[i], "--rotate") && i + 1 < argc) {
            const char *r = argv[++i];
            rotate = !strcmp(r, "orbit") ? APTGPU_ROTATE_ORBIT : !strcmp(r, "yes") ? APTGPU_ROTATE_YES : APTGPU_ROTATE_NO;
        }
    }

    /* the palette, decoded by the caller (the reference: image::open(..).into_rgb8(), processing.rs:115) */
    static uint8_t palette[256 * 256 * 3];
    aptgpu_color_settings color;
    memset(&color, 0, sizeof color);
    color.struct_size = sizeof color;
    color.palette_rgb = palette;
    if (lab) color.flags = APTGPU_COLOR_EQUALIZE_LAB;
    if (palette_path) {
        FILE *p = fopen(palette_path, "rb");
        if (!p || fread(palette, 1, sizeof palette, p) != sizeof palette || fgetc(p) != EOF) {
            fprintf(stderr, "Invalid palette image dimensions (want %u raw RGB bytes): %s\n", (unsigned)sizeof palette,
                    palette_path);
            return 1;
        }
        fclose(p);
    }

    /* the file image */
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char *bytes = malloc(n > 0 ? (size_t)n : 1);
    if (!bytes || fread(bytes, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "read error\n"); return 1; }
    fclose(f);

    /* the `standard` profile (default_settings.toml:108-116) */
    aptgpu_settings settings;
    memset(&settings, 0, sizeof settings);
    settings.work_rate = 12480;
    settings.resample_atten = 30.f;
    settings.resample_delta_freq = 1000.f;
    settings.resample_cutout = 4800.f;
    settings.demodulation_atten = 25.f;

    aptgpu_context ctx;
    memset(&ctx, 0, sizeof ctx);
    ctx.status = on_status;
    ctx.mode = APTGPU_MODE_STRICT;

    char err[1024] = "";
    float *rows = NULL;
    size_t n_rows_px = 0;
    aptgpu_stats stats;
    uint32_t rate = 0;
    int rc;
    /* --track=W,LAMBDA[,LAG]: read once; LAG belongs to the live tracker, and raw IQ is tracked as a live stream only */
    aptgpu_live_track_settings lt = {sizeof(aptgpu_live_track_settings), 8, 8, 0.1f};
    if (flywheel) {
        const int fields = *flywheel ? sscanf(flywheel, "%u,%f,%u", &lt.max_jitter, &lt.penalty, &lt.lag_rows) : 2;
        if (fields < 2) {
            fprintf(stderr, "--track=W,LAMBDA[,LAG]: cannot read \"%s\"\n", flywheel);
            return 2;
        }
        if (fields == 3 && live_seconds <= 0.0) {
            fprintf(stderr, "--track=W,LAMBDA,LAG: LAG is the live tracker's decision lag and needs --live SECONDS\n");
            return 2;
        }
        if (iq_spec && live_seconds <= 0.0) {
            fprintf(stderr, "--iq with --track=: raw IQ is tracked as a live stream only; add --live SECONDS\n");
            return 2;
        }
    }
    if (afc && (!iq_spec || live_seconds > 0.0)) {
        fprintf(stderr, "--afc follows the carrier of a whole IQ recording: it needs --iq and excludes --live\n");
        return 2;
    }
    if (iq_spec) {
        /* raw IQ frames: FM demodulation in front of the decode, in one piece or as a live stream */
        aptgpu_fm_settings fs;
        aptgpu_fm_default_settings(&fs);
        char fmt[8] = "";
        unsigned fs_hz = 0, dec = 0;
        double shift = 0.0;
        if (sscanf(iq_spec, "%7[^:]:%u:%u:%lf", fmt, &fs_hz, &dec, &shift) < 3) {
            fprintf(stderr, "--iq FMT:FS:D[:SHIFT_HZ]: cannot read \"%s\"\n", iq_spec);
            return 2;
        }
        fs.format = !strcmp(fmt, "u8") ? APTGPU_IQ_U8 : !strcmp(fmt, "s8") ? APTGPU_IQ_S8 : !strcmp(fmt, "s16") ? APTGPU_IQ_S16
                    : !strcmp(fmt, "f32") ? APTGPU_IQ_F32 : -1;
        fs.sample_rate_hz = fs_hz;
        fs.decimation = dec;
        fs.shift_hz = shift;
        const size_t frame_bytes = fs.format == APTGPU_IQ_S16 ? 4 : fs.format == APTGPU_IQ_F32 ? 8 : 2;
        const size_t n_frames = (size_t)n / frame_bytes;  /* (a trailing partial frame is dropped) */
        memset(&stats, 0, sizeof stats);
        if (live_seconds > 0.0) {
            aptgpu_iq_live_settings ls;
            memset(&ls, 0, sizeof ls);
            ls.struct_size = sizeof ls;
            ls.sync = sync;
            aptgpu_iq_live *live = NULL;
            rc = flywheel ? aptgpu_iq_live_create_tracked(&ctx, &settings, &fs, &ls, &lt, &live, err, sizeof err)
                          : aptgpu_iq_live_create(&ctx, &settings, &fs, &ls, &live, err, sizeof err);
            if (rc != APTGPU_OK) { fprintf(stderr, "iq live failed (%d): %s\n", rc, err); return 1; }
            size_t chunk = (size_t)(live_seconds * fs_hz);
            if (chunk == 0) chunk = 1;
            aptgpu_stream_result sr;
            memset(&sr, 0, sizeof sr);
            sr.struct_size = sizeof sr;
            size_t n_rows = 0, pushes = 0;
            for (size_t at = 0; rc == APTGPU_OK; at += chunk, ++pushes) {
                const int last = at >= n_frames;  /* the call after the last chunk is the finish */
                const size_t take = last ? 0 : (n_frames - at < chunk ? n_frames - at : chunk);
                const size_t cap = aptgpu_iq_live_rows_bound(live, take);
                float *grown = realloc(rows, (n_rows + cap + 1) * 2080 * sizeof(float));
                uint64_t *pos = malloc((cap + 1) * sizeof(uint64_t));
                if (!grown || !pos) { fprintf(stderr, "out of memory\n"); return 1; }
                rows = grown;
                rc = last ? aptgpu_iq_live_finish(live, rows + n_rows * 2080, pos, cap, &sr, err, sizeof err)
                          : aptgpu_iq_live_push(live, bytes + at * frame_bytes, take, rows + n_rows * 2080, pos, cap, &sr, err,
                                                sizeof err);
                free(pos);
                if (rc == APTGPU_OK) n_rows += sr.n_rows;
                if (last) break;
            }
            aptgpu_stream_track_result tr;
            memset(&tr, 0, sizeof tr);
            tr.struct_size = sizeof tr;
            if (flywheel && rc == APTGPU_OK) rc = aptgpu_iq_live_track_results(live, &tr, err, sizeof err);
            if (flywheel && rc == APTGPU_OK)
                fprintf(stderr, "tracked live: %llu row starts %u rows behind the best survivor (jitter %u, penalty %g), %u relocks\n",
                        (unsigned long long)tr.n_positions, lt.lag_rows, lt.max_jitter, lt.penalty, tr.n_relocks);
            aptgpu_iq_live_destroy(live);
            free(bytes);
            if (rc != APTGPU_OK) { fprintf(stderr, "live decode failed (%d): %s\n", rc, err); return 1; }
            n_rows_px = n_rows * 2080;
            rate = fs_hz / (dec ? dec : 1);
            fprintf(stderr, "%u Hz audio from %u Hz IQ, %llu sync frames, %llu rows from %llu pushes of %g s\n", rate, fs_hz,
                    (unsigned long long)sr.n_sync, (unsigned long long)n_rows, (unsigned long long)pushes, live_seconds);
        } else {
            float *audio = NULL;
            size_t n_audio = 0;
            if (afc) {
                /* the carrier is not where SHIFT_HZ says: estimate it per block, demodulate with an NCO that follows */
                aptgpu_afc_settings as;
                aptgpu_fm_afc_default_settings(&as);
                as.max_offset_hz = (float)afc_max_hz;
                aptgpu_afc_record *table = NULL;
                uint8_t *good = NULL;
                size_t n_blocks = 0, n_good = 0;
                rc = aptgpu_fm_demodulate_afc(&ctx, &fs, &as, bytes, n_frames, &audio, &n_audio, &rate, &table, NULL, &good,
                                              &n_blocks, err, sizeof err);
                if (rc == APTGPU_OK && n_blocks) {
                    const size_t at[3] = {0, n_blocks / 2, n_blocks - 1};
                    double hz[3];
                    for (int k = 0; k < 3; ++k) hz[k] = (double)(int32_t)table[at[k]].pw * fs_hz / 4294967296.0;
                    for (size_t b = 0; b < n_blocks; ++b) n_good += good[b];
                    fprintf(stderr, "afc: carrier at %+.0f Hz, %+.0f Hz, %+.0f Hz (start, middle, end); %llu of %llu blocks good\n",
                            hz[0], hz[1], hz[2], (unsigned long long)n_good, (unsigned long long)n_blocks);
                }
                aptgpu_free(table);
                aptgpu_free(good);
            } else {
                rc = aptgpu_fm_demodulate(&ctx, &fs, bytes, n_frames, &audio, &n_audio, &rate, err, sizeof err);
            }
            free(bytes);
            if (rc != APTGPU_OK) { fprintf(stderr, "fm demodulation failed (%d): %s\n", rc, err); return 1; }
            rc = aptgpu_decode(&ctx, &settings, audio, n_audio, rate, sync, &rows, &n_rows_px, &stats, err, sizeof err);
            aptgpu_free(audio);
            if (rc != APTGPU_OK) { fprintf(stderr, "decode failed (%d): %s\n", rc, err); return 1; }
            fprintf(stderr, "%u Hz audio from %u Hz IQ, %llu sync frames, %llu rows\n", rate, fs_hz,
                    (unsigned long long)stats.n_sync, (unsigned long long)(n_rows_px / 2080));
        }
    } else if (flywheel && live_seconds <= 0.0) {
        /* load -> front end -> flywheel sync: the rows of the tracked path, with each row's lock indicator */
        aptgpu_track_settings ts = {sizeof(aptgpu_track_settings), lt.max_jitter, lt.penalty, 0};
        float *signal = NULL, *scores = NULL;
        size_t n_signal = 0;
        aptgpu_wav_spec spec;
        rc = aptgpu_load_wav(&ctx, bytes, (size_t)n, &signal, &n_signal, &rate, &spec, err, sizeof err);
        if (rc != APTGPU_OK) { fprintf(stderr, "load failed (%d): %s\n", rc, err); return 1; }
        aptgpu_track_result tr;
        memset(&tr, 0, sizeof tr);
        tr.struct_size = sizeof tr;
        rc = aptgpu_decode_tracked(&ctx, &settings, signal, n_signal, rate, &ts, &rows, &n_rows_px, NULL, &scores, &tr, err,
                                   sizeof err);
        aptgpu_free(signal);
        free(bytes);
        if (rc != APTGPU_OK) { fprintf(stderr, "tracked decode failed (%d): %s\n", rc, err); return 1; }
        unsigned locked = 0;
        for (uint32_t k = 0; k < tr.n_positions; ++k) locked += scores[k] > 0.5f;
        aptgpu_free(scores);
        memset(&stats, 0, sizeof stats);
        fprintf(stderr, "%u Hz, tracked %u row starts (jitter %u, penalty %g), %u with a score above 0.5, %llu rows\n", rate,
                tr.n_positions, ts.max_jitter, ts.penalty, locked, (unsigned long long)(n_rows_px / 2080));
    } else if (live_seconds > 0.0) {
        /* load, then the samples in chunks through a stream: each push returns the rows that became final */
        float *signal = NULL;
        size_t n_signal = 0;
        aptgpu_wav_spec spec;
        rc = aptgpu_load_wav(&ctx, bytes, (size_t)n, &signal, &n_signal, &rate, &spec, err, sizeof err);
        free(bytes);
        if (rc != APTGPU_OK) { fprintf(stderr, "load failed (%d): %s\n", rc, err); return 1; }
        aptgpu_stream_settings ss;
        memset(&ss, 0, sizeof ss);
        ss.struct_size = sizeof ss;
        ss.input_rate_hz = rate;
        ss.sync = sync;
        ss.format = APTGPU_STREAM_F32;
        aptgpu_stream *stream = NULL;
        /* with --track=W,LAMBDA[,LAG]: the same stream with the flywheel tracker in the picker's place */
        rc = flywheel ? aptgpu_stream_create_tracked(&ctx, &settings, &ss, &lt, &stream, err, sizeof err)
                      : aptgpu_stream_create(&ctx, &settings, &ss, &stream, err, sizeof err);
        if (rc != APTGPU_OK) { fprintf(stderr, "stream failed (%d): %s\n", rc, err); return 1; }
        size_t chunk = (size_t)(live_seconds * rate);
        if (chunk == 0) chunk = 1;
        aptgpu_stream_result sr;
        memset(&sr, 0, sizeof sr);
        sr.struct_size = sizeof sr;
        size_t n_rows = 0, pushes = 0;
        for (size_t at = 0; rc == APTGPU_OK; at += chunk, ++pushes) {
            const int last = at >= n_signal;  /* the call after the last chunk is the finish */
            const size_t take = last ? 0 : (n_signal - at < chunk ? n_signal - at : chunk);
            const size_t cap = aptgpu_stream_rows_bound(stream, take);
            float *grown = realloc(rows, (n_rows + cap) * 2080 * sizeof(float));
            uint64_t *pos = malloc(cap * sizeof(uint64_t));
            if (!grown || !pos) { fprintf(stderr, "out of memory\n"); return 1; }
            rows = grown;
            rc = last ? aptgpu_stream_finish(stream, rows + n_rows * 2080, pos, cap, &sr, err, sizeof err)
                      : aptgpu_stream_push(stream, signal + at, take, rows + n_rows * 2080, pos, cap, &sr, err, sizeof err);
            free(pos);
            if (rc == APTGPU_OK) n_rows += sr.n_rows;
            if (last) break;
        }
        aptgpu_stream_track_result tr;
        memset(&tr, 0, sizeof tr);
        tr.struct_size = sizeof tr;
        if (flywheel && rc == APTGPU_OK) rc = aptgpu_stream_track_results(stream, &tr, err, sizeof err);
        aptgpu_stream_destroy(stream);
        aptgpu_free(signal);
        if (rc != APTGPU_OK) { fprintf(stderr, "live decode failed (%d): %s\n", rc, err); return 1; }
        n_rows_px = n_rows * 2080;
        memset(&stats, 0, sizeof stats);
        if (flywheel)
            fprintf(stderr, "tracked live: %llu row starts %u rows behind the best survivor (jitter %u, penalty %g), %u relocks\n",
                    (unsigned long long)tr.n_positions, lt.lag_rows, lt.max_jitter, lt.penalty, tr.n_relocks);
        fprintf(stderr, "%u Hz, %llu sync frames, %llu rows from %llu pushes of %g s\n", rate, (unsigned long long)sr.n_sync,
                (unsigned long long)n_rows, (unsigned long long)pushes, live_seconds);
    } else {
    rc = aptgpu_decode_wav(&ctx, &settings, bytes, (size_t)n, sync, &rows, &n_rows_px, &stats, &rate, err,
                               sizeof err);
    free(bytes);
    if (rc != APTGPU_OK) { fprintf(stderr, "decode failed (%d): %s\n", rc, err); return 1; }
    fprintf(stderr, "%u Hz, %llu sync frames, %llu rows\n", rate, (unsigned long long)stats.n_sync,
            (unsigned long long)(n_rows_px / 2080));
    }

    if (despeckle) {
        /* on the f32 rows, before any contrast limit is taken from them */
        aptgpu_despeckle_settings ds = {sizeof(aptgpu_despeckle_settings), atoi(despeckle), 0.f};
        const char *colon = strchr(despeckle, ':');
        if (colon) ds.threshold = (float)atof(colon + 1);
        aptgpu_despeckle_result dr;
        float *filtered = NULL;
        rc = aptgpu_despeckle(&ctx, rows, n_rows_px, &ds, &filtered, &dr, err, sizeof err);
        if (rc != APTGPU_OK) { fprintf(stderr, "despeckle failed (%d): %s\n", rc, err); return 1; }
        fprintf(stderr, "despeckle: radius %d, %llu of %llu samples replaced (t = %g)\n", ds.radius,
                (unsigned long long)dr.replaced, (unsigned long long)dr.height * 2080ull, dr.t);
        aptgpu_free(rows);
        rows = filtered;
    }

    if (sun) {
        /* on the f32 rows, in front of the image stage: the visible channel normalised by the sun's elevation */
        const size_t height = n_rows_px / 2080;
        aptgpu_geoloc_settings gs;
        memset(&gs, 0, sizeof gs);
        gs.struct_size = sizeof gs;
        gs.channel = sun[0] == 'B' ? 1 : 0;
        gs.time_kind = APTGPU_REF_TIME_START;
        gs.max_zenith_deg = 80.f;
        const char *colon = strchr(sun + 2, ':');
        double *track = malloc((height ? height : 1) * 2 * sizeof(double));
        FILE *t = track_path ? fopen(track_path, "rb") : NULL;
        if ((sun[0] != 'A' && sun[0] != 'B') || sun[1] != ':' || !track || !t ||
            fread(track, sizeof(double), 2 * height, t) != 2 * height || fgetc(t) != EOF) {
            fprintf(stderr, "--sun A|B:UNIX_MS[:BLACK] needs --track FILE with exactly %zu (lat, lon) f64 pairs\n", height);
            return 1;
        }
        fclose(t);
        gs.unix_ms = atoll(sun + 2);
        if (colon) {
            gs.black_level = (float)atof(colon + 1);
        } else {
            aptgpu_image_result tel;
            rc = aptgpu_read_telemetry(&ctx, rows, n_rows_px, &tel, err, sizeof err);
            if (rc != APTGPU_OK) { fprintf(stderr, "--sun: no telemetry for the black level (%d): %s\n", rc, err); return 1; }
            gs.black_level = gs.channel ? tel.values_b[8] : tel.values_a[8];
        }
        aptgpu_geoloc_result gr;
        memset(&gr, 0, sizeof gr);
        gr.struct_size = sizeof gr;
        float *normalised = NULL;
        rc = aptgpu_geolocate(&ctx, rows, n_rows_px, track, height, NULL, NULL, &gs, NULL, NULL, &normalised, &gr, err,
                              sizeof err);
        free(track);
        if (rc != APTGPU_OK) { fprintf(stderr, "sun normalisation failed (%d): %s\n", rc, err); return 1; }
        fprintf(stderr, "sun: channel %c, black %g, cos(zenith) %.3f .. %.3f, %llu of %llu pixels capped at 80 degrees\n",
                sun[0], gs.black_level, gr.cos_min, gr.cos_max, (unsigned long long)gr.n_capped,
                (unsigned long long)gr.height * 909ull);
        aptgpu_free(rows);
        rows = normalised;
    }

    if (land_dir) {
        /* the land / sea / lake mask of the swath (aptgpu_land_mask) from DIR/countries.shp and DIR/lakes.shp, written as
         * a 909-wide PGM of the classes 0 sea, 1 land, 2 lake, 255 invalid instead of the image */
        const size_t height = n_rows_px / 2080;
        int failed = 1;
        double *track = malloc((height ? height : 1) * 2 * sizeof(double));
        FILE *t = track_path ? fopen(track_path, "rb") : NULL;
        aptgpu_map_layers *layers = NULL;
        uint8_t *mask = NULL;
        FILE *out = NULL;
        if (!track || !t || fread(track, sizeof(double), 2 * height, t) != 2 * height || fgetc(t) != EOF) {
            fprintf(stderr, "--land-mask DIR needs --track FILE with exactly %zu (lat, lon) f64 pairs\n", height);
            goto land_done;
        }
        if (aptgpu_map_layers_create(&layers) != APTGPU_OK) goto land_done;
        {
            const char *files[2] = {"countries.shp", "lakes.shp"};
            const int which[2] = {APTGPU_MAP_COUNTRIES, APTGPU_MAP_LAKES};
            for (int k = 0; k < 2; k++) {
                char path[4096];
                double *xy = NULL;
                uint32_t *parts = NULL;
                size_t n_points = 0, n_parts = 0;
                snprintf(path, sizeof path, "%s/%s", land_dir, files[k]);
                rc = aptgpu_map_read_shapefile(path, 5, &xy, &n_points, &parts, &n_parts, err, sizeof err);
                if (rc == APTGPU_OK) rc = aptgpu_map_layers_set(layers, which[k], xy, n_points, parts, n_parts, err, sizeof err);
                aptgpu_free(xy);
                aptgpu_free(parts);
                if (rc != APTGPU_OK) { fprintf(stderr, "--land-mask: %s (%d): %s\n", path, rc, err); goto land_done; }
            }
        }
        {
            aptgpu_land_mask_result lr;
            memset(&lr, 0, sizeof lr);
            lr.struct_size = sizeof lr;
            rc = aptgpu_land_mask(&ctx, height, track, height, NULL, NULL, layers, NULL, &mask, &lr, err, sizeof err);
            if (rc != APTGPU_OK) { fprintf(stderr, "land mask failed (%d): %s\n", rc, err); goto land_done; }
            fprintf(stderr, "land mask: %llu sea, %llu land, %llu lake, %llu invalid of %zu rows x 909\n",
                    (unsigned long long)lr.n_sea, (unsigned long long)lr.n_land, (unsigned long long)lr.n_lake,
                    (unsigned long long)lr.n_invalid, height);
        }
        out = fopen(argv[2], "wb");
        if (!out) { perror(argv[2]); goto land_done; }
        if (fprintf(out, "P5\n909 %zu\n255\n", height) < 0 || fwrite(mask, 1, height * 909, out) != height * 909) {
            fprintf(stderr, "%s: short write\n", argv[2]);
            goto land_done;
        }
        failed = 0;
    land_done:
        if (out && fclose(out) != 0 && !failed) { perror(argv[2]); failed = 1; }
        if (t) fclose(t);
        free(track);
        aptgpu_map_layers_destroy(layers);
        aptgpu_free(mask);
        aptgpu_free(rows);
        return failed;
    }

    uint8_t *image = NULL;
    size_t n_px = 0;
    aptgpu_image_result info;
    const int rgba = palette_path || map_dir;
    aptgpu_png_settings ps = {sizeof(aptgpu_png_settings), 0};
    aptgpu_projection_settings proj;
    memset(&proj, 0, sizeof proj);
    if (project) {
        /* the georeferenced image: the grid is fitted to the track, which comes from --track or from the TLE */
        const size_t height = n_rows_px / 2080;
        const int kind = !strncmp(project, "mercator", 8) ? APTGPU_PROJECTION_MERCATOR : APTGPU_PROJECTION_EQUIRECTANGULAR;
        const char *colon = strchr(project, ':');
        const double step = colon ? atof(colon + 1) : 0.04;
        double *track = malloc((height ? height : 1) * 2 * sizeof(double));
        char *tle = NULL;
        aptgpu_orbit_settings os;
        memset(&os, 0, sizeof os);
        rc = APTGPU_OK;
        if (tle_path) {
            FILE *t = fopen(tle_path, "rb");
            long tn = 0;
            if (t) { fseek(t, 0, SEEK_END); tn = ftell(t); fseek(t, 0, SEEK_SET); tle = malloc((size_t)tn + 1); }
            if (!t || !tle || fread(tle, 1, (size_t)tn, t) != (size_t)tn || !sat || ref_kind < 0) {
                fprintf(stderr, "--tle FILE needs a readable file, --sat NAME and --start-ms N or --end-ms N\n");
                return 1;
            }
            tle[tn] = 0;
            fclose(t);
            os.struct_size = sizeof os;
            os.sat_name = sat;
            os.tle = tle;
            os.ref_kind = ref_kind;
            os.ref_unix_ms = ref_ms;
            rc = aptgpu_sat_track_host(&os, (uint32_t)height, track, err, sizeof err);  /* for the fit alone */
        } else {
            FILE *t = track_path ? fopen(track_path, "rb") : NULL;
            if (!track || !t || fread(track, sizeof(double), 2 * height, t) != 2 * height || fgetc(t) != EOF) {
                fprintf(stderr, "--project needs --track FILE with exactly %zu (lat, lon) f64 pairs, or --tle\n", height);
                return 1;
            }
            fclose(t);
        }
        aptgpu_map_layers *layers = NULL;
        aptgpu_map_settings ms = {sizeof(aptgpu_map_settings), 0, 0.0, 1.0, 1.0};  /* config.rs:646-648 */
        if (rc == APTGPU_OK) rc = aptgpu_projection_fit(track, height, ms.hscale, kind, step, 0, &proj, err, sizeof err);
        proj.sampling = APTGPU_SAMPLING_BILINEAR;
        proj.grid_deg = grid_deg;
        proj.grid_color[0] = proj.grid_color[1] = proj.grid_color[2] = 255;
        proj.grid_color[3] = 160;
        if (rc == APTGPU_OK && map_dir) {
            rc = aptgpu_map_layers_create(&layers);
            if (rc == APTGPU_OK) rc = aptgpu_map_layers_load_dir(layers, map_dir, err, sizeof err);
        }
        if (rc == APTGPU_OK)
            rc = aptgpu_process_image_project(&ctx, rows, n_rows_px, contrast, 0.98f, rotate,
                                              palette_path ? &color : NULL, rgba ? 4 : 1, &ms, layers,
                                              tle_path ? NULL : track, tle_path ? &os : NULL, &proj,
                                              png ? APTGPU_OUTPUT_PNG : APTGPU_OUTPUT_PIXELS, &ps, &image, &n_px, &info,
                                              err, sizeof err);
        aptgpu_map_layers_destroy(layers);
        free(track);
        free(tle);
    } else if (tle_path) {
        /* OrbitSettings: the track (and Rotate::Orbit) from the TLE, computed by the library; no track file */
        char *tle = NULL;
        FILE *t = fopen(tle_path, "rb");
        long tn = 0;
        if (t) { fseek(t, 0, SEEK_END); tn = ftell(t); fseek(t, 0, SEEK_SET); tle = malloc((size_t)tn + 1); }
        if (!t || !tle || fread(tle, 1, (size_t)tn, t) != (size_t)tn || !sat || ref_kind < 0) {
            fprintf(stderr, "--tle FILE needs a readable file, --sat NAME and --start-ms N or --end-ms N\n");
            return 1;
        }
        tle[tn] = 0;
        fclose(t);
        aptgpu_map_layers *layers = NULL;
        aptgpu_map_settings ms = {sizeof(aptgpu_map_settings), 0, 0.0, 1.0, 1.0};  /* config.rs:646-648 */
        aptgpu_orbit_settings os;
        memset(&os, 0, sizeof os);
        os.struct_size = sizeof os;
        os.sat_name = sat;
        os.tle = tle;
        os.ref_kind = ref_kind;
        os.ref_unix_ms = ref_ms;
        os.draw_map = map_dir ? &ms : NULL;
        rc = APTGPU_OK;
        if (map_dir) {
            rc = aptgpu_map_layers_create(&layers);
            if (rc == APTGPU_OK) rc = aptgpu_map_layers_load_dir(layers, map_dir, err, sizeof err);
        }
        if (rc == APTGPU_OK)
            rc = aptgpu_process_image_orbit(&ctx, rows, n_rows_px, contrast, 0.98f, rotate,
                                            palette_path ? &color : NULL, rgba ? 4 : 1, &os, layers,
                                            png ? APTGPU_OUTPUT_PNG : APTGPU_OUTPUT_PIXELS, &ps, &image, &n_px, &info,
                                            err, sizeof err);
        aptgpu_map_layers_destroy(layers);
        free(tle);
    } else if (rotate == APTGPU_ROTATE_ORBIT) {
        fprintf(stderr, "--rotate orbit needs --tle FILE --sat NAME and a time\n");
        return 1;
    } else if (map_dir) {
        /* the track: one (lat, lon) per image row, as map.rs:41-58 computes it with SGP4; with --fit the long one,
         * margin_rows rows more at either end */
        const size_t height = n_rows_px / 2080;
        aptgpu_fit_settings fs;
        aptgpu_fit_default_settings(&fs);
        const size_t margin = fit ? (size_t)fs.margin_rows : 0, track_rows = height + 2 * margin;
        double *track_buf = malloc((track_rows ? track_rows : 1) * 2 * sizeof(double));
        FILE *t = track_path ? fopen(track_path, "rb") : NULL;
        if (!track_buf || !t || fread(track_buf, sizeof(double), 2 * track_rows, t) != 2 * track_rows || fgetc(t) != EOF) {
            fprintf(stderr, "--map%s needs --track FILE with exactly %zu (lat, lon) f64 pairs\n", fit ? " --fit" : "", track_rows);
            return 1;
        }
        fclose(t);
        const double *track = track_buf + 2 * margin;
        aptgpu_map_layers *layers = NULL;
        aptgpu_map_settings ms = {sizeof(aptgpu_map_settings), 0, 0.0, 1.0, 1.0};  /* config.rs:646-648 */
        rc = aptgpu_map_layers_create(&layers);
        if (rc == APTGPU_OK) rc = aptgpu_map_layers_load_dir(layers, map_dir, err, sizeof err);
        if (rc == APTGPU_OK && fit) {
            /* --fit: yaw, scales and the time offset from the image itself (the unrotated gray image against the
             * layers' lines), then the overlay with what was found */
            uint8_t *gray = NULL;
            size_t n_gray = 0;
            aptgpu_image_result gi;
            aptgpu_fit_result fr;
            memset(&fr, 0, sizeof fr);
            fr.struct_size = sizeof fr;
            rc = aptgpu_process_gray(&ctx, rows, n_rows_px, contrast, 0.98f, APTGPU_ROTATE_NO, &gray, &n_gray, &gi, err,
                                     sizeof err);
            if (rc == APTGPU_OK)
                rc = aptgpu_fit_overlay(&ctx, gray, height, track_buf, track_rows, NULL, layers, &ms, &fs, &fr, NULL, NULL,
                                        err, sizeof err);
            aptgpu_free(gray);
            if (rc == APTGPU_OK) {
                fprintf(stderr, "fit: yaw %g, hscale %g, vscale %g, %d rows = %lld ms (q %g over %u points%s)\n", fr.yaw,
                        fr.hscale, fr.vscale, fr.shift_rows, (long long)fr.time_offset_ms, fr.q, fr.count,
                        fr.reason == APTGPU_FIT_REASON_FLAT ? "; a flat image: the initial settings" : "");
                ms.yaw = fr.yaw;
                ms.hscale = fr.hscale;
                ms.vscale = fr.vscale;
                track = track_buf + 2 * (size_t)((long long)margin + fr.shift_rows);
            }
        }
        if (rc == APTGPU_OK && png)
            rc = aptgpu_process_image_png(&ctx, rows, n_rows_px, contrast, 0.98f, rotate,
                                          palette_path ? &color : NULL, 4, &ms, layers, track, &ps, &image, &n_px,
                                          &info, err, sizeof err);
        else if (rc == APTGPU_OK)
            rc = aptgpu_process_image_map(&ctx, rows, n_rows_px, contrast, 0.98f, rotate,
                                          palette_path ? &color : NULL, 4, &ms, layers, track, &image, &n_px, &info,
                                          err, sizeof err);
        aptgpu_map_layers_destroy(layers);
        free(track_buf);
    } else if (png)
        rc = aptgpu_process_image_png(&ctx, rows, n_rows_px, contrast, 0.98f, rotate,
                                      palette_path ? &color : NULL, palette_path ? 4 : 1, NULL, NULL, NULL, &ps, &image,
                                      &n_px, &info, err, sizeof err);
    else if (palette_path || contrast == APTGPU_CONTRAST_HISTOGRAM || contrast == APTGPU_CONTRAST_HISTOGRAM_FLOAT)
        rc = aptgpu_process_image(&ctx, rows, n_rows_px, contrast, 0.98f, rotate,
                                  palette_path ? &color : NULL, palette_path ? 4 : 1, &image, &n_px, &info, err,
                                  sizeof err);
    else
        rc = aptgpu_process_gray(&ctx, rows, n_rows_px, contrast, 0.98f, rotate, &image, &n_px, &info,
                                 err, sizeof err);
    aptgpu_free(rows);
    if (rc != APTGPU_OK) { fprintf(stderr, "image stage failed (%d): %s\n", rc, err); return 1; }

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 1; }
    if (png) {
        fwrite(image, 1, n_px, o);  /* the file as it is: img.save(&output_filename), main.rs */
    } else if (project) {
        fprintf(o, "P6\n%u %u\n255\n", proj.width, proj.height);
        for (size_t i = 0; i < (size_t)proj.width * proj.height; ++i) fwrite(image + 4 * i, 1, 3, o);  /* drop alpha */
    } else if (rgba) {
        fprintf(o, "P6\n2080 %u\n255\n", info.height);
        for (size_t i = 0; i < (size_t)info.height * 2080u; ++i) fwrite(image + 4 * i, 1, 3, o);  /* drop alpha */
    } else {
        fprintf(o, "P5\n2080 %u\n255\n", info.height);
        fwrite(image, 1, (size_t)info.height * 2080u, o);
    }
    fclose(o);
    aptgpu_free(image);
    if (project)
        fprintf(stderr, "wrote %s: %u x %u, north %g, west %g, %g degrees per pixel\n", argv[2], proj.width, proj.height,
                proj.lat_north, proj.lon_west, proj.step);
    else
        fprintf(stderr, "wrote %s: 2080 x %u, contrast limits %g .. %g\n", argv[2], info.height, info.low, info.high);
    return 0;
}
