// process_baseband's log (header-only: the second reader and the loop both write to it)
#ifndef PB_HOST_LOG_H
#define PB_HOST_LOG_H

#include <sys/stat.h>
#include <unistd.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

namespace host {

// multilog stand-in: timestamped lines to the per-process log file and optionally stdout
struct Log {
    std::vector<FILE *> fps;
    void open(const std::string &logdir, bool to_stdout)
    {
        char stamp[32], host[256] = "host";
        time_t t = time(nullptr);
        tm g;
        gmtime_r(&t, &g);
        strftime(stamp, sizeof stamp, "%Y%m%d_%H%M%S", &g);
        gethostname(host, sizeof host - 1);
        mkdir(logdir.c_str(), 0777);
        char path[1024];
        snprintf(path, sizeof path, "%s/%s_%s_process_%06d.log", logdir.c_str(), stamp, host, (int)getpid());
        if (FILE *fp = fopen(path, "w")) fps.push_back(fp);
        if (to_stdout) fps.push_back(stdout);
    }
    void line(bool err, const char *fmt, ...) __attribute__((format(printf, 3, 4)))
    {
        char msg[2048], stamp[32];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof msg, fmt, ap);
        va_end(ap);
        time_t t = time(nullptr);
        tm g;
        gmtime_r(&t, &g);
        strftime(stamp, sizeof stamp, "%Y-%m-%d-%H:%M:%S", &g);
        const size_t n = strlen(msg);
        for (FILE *fp : fps) {
            fprintf(fp, "[%s] %s%s%s", stamp, err ? "ERR: " : "", msg, (n && msg[n - 1] == '\n') ? "" : "\n");
            fflush(fp);
        }
    }
};

}   // namespace host

#endif
